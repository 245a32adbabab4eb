// What the checked batch verifier (proto::VerifyBatchChecked, curdle_verify_batch_checked) and the backend that runs
// its point check say to each other.  The backend (csrc/check_api.hip) includes this and nothing else of the
// protocol layer; the host layer names no backend symbol, so the host-only build links without the check.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <functional>

#include "../../include/curdle_msm.h"

namespace curdle {
namespace proto {
using PointFault = curdle_point_fault;  // code (CURDLE_DECODE_*), vector (0 Rs, 1 Ss, 2 Ts, 3 Us, 4 M), index in the vector
using ChunkCheckFn = std::function<int(const uint64_t* const* affine_vecs, const size_t* lens, size_t na,
                                       const uint64_t* const* jac_points, size_t nj, uint8_t* affine_status, uint8_t* jac_status)>;
}  // namespace proto
}  // namespace curdle

// curdle_verify_batch_checked behind its argument checks (host/proto_api.cpp): the unchecked call's sharding over
// contexts, with `check` run on the context of the shard.  stats[0] += members rejected by the check, stats[1] +=
// chunks checked.
int curdle_verify_batch_checked_with(const curdle_crs* crs, size_t k, const uint8_t* const* proofs, const size_t* proof_lens,
                                     const uint64_t* const* Rs, const uint64_t* const* Ss, const uint64_t* const* Ts,
                                     const uint64_t* const* Us, size_t ell, const uint64_t* Ms, curdle_rand* rand, int nthreads,
                                     int* oks, curdle_point_fault* faults, const curdle::proto::ChunkCheckFn& check,
                                     unsigned long long stats[2]);
