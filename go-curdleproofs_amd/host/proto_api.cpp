// C ABI of the host-side protocol restatement (curdleproofs.h): CRS, the shuffle
// instance, curdleproof.Prove / Verify on serialised proofs.  Declared in
// include/curdle_msm.h under "Protocol layers".
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <exception>
#include <memory>
#include <new>
#include <stdexcept>
#include <thread>
#include <vector>

#include "../../include/curdle_msm.h"
#include "curdleproofs.h"
#include "device_accumulator.h"
#include "knobs.h"
#include "whisk.h"

using namespace curdle;
using alg::Point;
using alg::Scalar;

// defined in csrc/msm_context.hip
extern "C" int curdle_set_last_error(int code, const char* msg);

struct curdle_rand {  // same layout as in csrc/misc_api.hip
  common::Rand r;
  explicit curdle_rand(uint64_t seed) : r(seed) {}
};
struct curdle_crs {
  proto::CRS crs;
};
struct curdle_proof {
  proto::Proof p;
};

static std::vector<G1Affine> Affines(const uint64_t* p, size_t n) {
  std::vector<G1Affine> v(n);
  if (n) memcpy(v.data(), p, n * 96);
  return v;
}

template <class F>
static int Guard(F&& f) {
  try {
    return f();
  } catch (const std::bad_alloc&) {
    return curdle_set_last_error(CURDLE_ENOMEM, "out of memory");
  } catch (const alg::MsmError& e) {
    // a device-side failure (no device, HIP error, out of device memory) carries the code of
    // the entry point that failed: "could not compute", never to be read as "reject"
    return curdle_set_last_error(e.rc == CURDLE_OK || e.rc == CURDLE_EINVAL ? CURDLE_EHIP : e.rc, e.what());
  } catch (const std::exception& e) {
    return curdle_set_last_error(CURDLE_EINVAL, e.what());  // malformed input / structural error of the protocol
  }
}

extern "C" curdle_crs* curdle_crs_generate(size_t ell, curdle_rand* rand) {
  if (!rand) return nullptr;
  try {
    curdle_crs* c = new curdle_crs();
    c->crs = proto::GenerateCRS(ell, rand->r);
    return c;
  } catch (...) {
    return nullptr;
  }
}
extern "C" void curdle_crs_free(curdle_crs* c) { delete c; }
extern "C" size_t curdle_crs_size(const curdle_crs* c) { return c ? c->crs.Gs.size() : 0; }

// ---------------------------------------------------------------------------------------------------------------------
// curdle_crs_from_points / _from_bytes / _export_points / _to_bytes: a CRS no curdle_rand produced.  The rule of a
// validated import is stated in include/curdle_msm.h; its per-point half is the device's (the three batched calls
// below, weak as host/algebra.cpp names device entry points: a host-only link builds and answers CURDLE_ENODEV), the
// duplicates and the sums are host work on ell + 7 public points.
// ---------------------------------------------------------------------------------------------------------------------
extern "C" int curdle_g1_check_batch(const uint64_t* points, size_t n, int subgroup_check, uint8_t* status) __attribute__((weak));
extern "C" int curdle_g1_check_jac_batch(const uint64_t* jac_points, size_t n, int subgroup_check, uint8_t* status)
    __attribute__((weak));
extern "C" int curdle_g1_decompress_batch(const uint8_t* in, size_t n, int subgroup_check, uint64_t* out_affine, uint8_t* status)
    __attribute__((weak));

namespace {
static_assert(proto::N_BLINDERS == CURDLE_CRS_N_BLINDERS, "the header's count of blinders");
constexpr size_t kCrsSingles = 5;  // H, Gt, Gu, Gsum, Hsum

struct CrsFields {  // the seven fields in wire order; Gs | Hs back to back
  std::vector<G1Affine> gens;  // ell + N_BLINDERS
  size_t ell = 0;
  Point H, Gt, Gu;
  G1Affine Gsum, Hsum;
};

// Where record `wire` of Gs | Hs | H | Gt | Gu | Gsum | Hsum lies, as the fault and the error text name it.
void CrsWhere(size_t wire, size_t ell, int* field, size_t* index) {
  if (wire < ell) {
    *field = CURDLE_CRS_GS;
    *index = wire;
  } else if (wire < ell + proto::N_BLINDERS) {
    *field = CURDLE_CRS_HS;
    *index = wire - ell;
  } else {
    *field = CURDLE_CRS_H + (int)(wire - ell - proto::N_BLINDERS);
    *index = 0;
  }
}
std::string CrsName(size_t wire, size_t ell) {
  static const char* const kField[7] = {"Gs", "Hs", "H", "Gt", "Gu", "Gsum", "Hsum"};
  int field;
  size_t index;
  CrsWhere(wire, ell, &field, &index);
  char buf[40];
  if (field <= CURDLE_CRS_HS)
    snprintf(buf, sizeof(buf), "%s[%zu]", kField[field], index);
  else
    snprintf(buf, sizeof(buf), "%s", kField[field]);
  return buf;
}
int CrsFault(size_t wire, size_t ell, int reason, const std::string& why, curdle_crs_fault* fault) {
  if (fault) {
    CrsWhere(wire, ell, &fault->field, &fault->index);
    fault->reason = reason;
  }
  return curdle_set_last_error(CURDLE_EINVAL, (CrsName(wire, ell) + ": " + why).c_str());
}

// The handle over the fields as they stand, and "no fault".
int CrsHandle(const CrsFields& f, curdle_crs** out, curdle_crs_fault* fault) {
  std::unique_ptr<curdle_crs> c(new curdle_crs());
  c->crs = proto::CRSFromPoints(std::vector<G1Affine>(f.gens.begin(), f.gens.begin() + f.ell),
                                std::vector<G1Affine>(f.gens.begin() + f.ell, f.gens.end()), f.H, f.Gt, f.Gu, f.Gsum, f.Hsum);
  *out = c.release();
  if (fault) *fault = curdle_crs_fault{-1, 0, 0};
  return CURDLE_OK;
}

// Steps 2 (the verdict over the device's status bytes, in wire order), 3 and 4 of a validated import, then the handle.
int CrsFinishValidated(CrsFields& f, const std::vector<uint8_t>& status, bool from_bytes, curdle_crs** out, curdle_crs_fault* fault) {
  const size_t ell = f.ell, n_gen = ell + proto::N_BLINDERS + 3;
  for (size_t w = 0; w < status.size(); w++) {
    const uint8_t st = status[w];
    if (st == CURDLE_DECODE_OK || (st == CURDLE_DECODE_INFINITY && w >= n_gen)) continue;
    const char* why = "invalid point";
    switch (st) {
      case CURDLE_DECODE_INFINITY: why = "the point at infinity is no generator"; break;
      case CURDLE_DECODE_BAD_ENCODING:
        why = from_bytes ? "not a valid compressed encoding" : "not a field element (a coordinate is not below p)";
        break;
      case CURDLE_DECODE_NOT_ON_CURVE: why = "not on the curve"; break;
      case CURDLE_DECODE_NOT_IN_SUBGROUP: why = "not in the prime-order subgroup"; break;
    }
    return CrsFault(w, ell, st, why, fault);
  }
  // duplicates: the canonical 96-byte records of the ell + 7 generators, sorted with their wire index; within a run of
  // equal records the second is the later point of the run's first pair, and the earliest such point is the fault
  std::vector<G1Affine> gen = f.gens;
  gen.push_back(f.H.Affine());
  gen.push_back(f.Gt.Affine());
  gen.push_back(f.Gu.Affine());
  std::vector<size_t> order(n_gen);
  for (size_t i = 0; i < n_gen; i++) order[i] = i;
  std::sort(order.begin(), order.end(), [&](size_t a, size_t b) {
    const int c = memcmp(&gen[a], &gen[b], sizeof(G1Affine));
    return c ? c < 0 : a < b;
  });
  size_t later = n_gen, earlier = 0;
  for (size_t i = 1; i < n_gen; i++)
    if (!memcmp(&gen[order[i - 1]], &gen[order[i]], sizeof(G1Affine)) &&
        (i < 2 || memcmp(&gen[order[i - 2]], &gen[order[i]], sizeof(G1Affine))) && order[i] < later) {
      later = order[i];
      earlier = order[i - 1];
    }
  if (later < n_gen)
    return CrsFault(later, ell, CURDLE_CRS_DUPLICATE,
                    "equal to " + CrsName(earlier, ell) + ": a known relation between generators", fault);
  // the sums, as GenerateCRS makes them (crs.go:41-48)
  Point gs = Point::Infinity(), hs = Point::Infinity();
  for (size_t i = 0; i < ell; i++) gs = gs + Point::FromAffine(f.gens[i]);
  for (size_t i = ell; i < ell + proto::N_BLINDERS; i++) hs = hs + Point::FromAffine(f.gens[i]);
  const G1Affine gsum = gs.Affine(), hsum = hs.Affine();
  if (memcmp(&gsum, &f.Gsum, sizeof(G1Affine))) return CrsFault(n_gen, ell, CURDLE_CRS_SUM_MISMATCH, "not the sum of Gs", fault);
  if (memcmp(&hsum, &f.Hsum, sizeof(G1Affine))) return CrsFault(n_gen + 1, ell, CURDLE_CRS_SUM_MISMATCH, "not the sum of Hs", fault);
  return CrsHandle(f, out, fault);
}

int CrsNoDevice(const char* who) {
  return curdle_set_last_error(CURDLE_ENODEV, (std::string(who) + ": the point checks of a validated import need the device backend").c_str());
}
}  // namespace

extern "C" int curdle_crs_from_points(const curdle_crs_points* in, unsigned flags, curdle_crs** out, curdle_crs_fault* fault) {
  if (out) *out = nullptr;
  if (!in || !out || !in->Gs || !in->Hs || !in->H || !in->Gt || !in->Gu || !in->Gsum || !in->Hsum)
    return curdle_set_last_error(CURDLE_EINVAL, "null argument");
  if (flags & ~CURDLE_CRS_TRUSTED) {
    char msg[64];
    snprintf(msg, sizeof(msg), "unknown flag bits 0x%x", flags & ~CURDLE_CRS_TRUSTED);
    return curdle_set_last_error(CURDLE_EINVAL, msg);
  }
  const size_t ell = in->ell;
  if (ell == 0 || ell > CURDLE_CRS_MAX_ELL) return curdle_set_last_error(CURDLE_EINVAL, "ell must be 1 ... 2^20 (CURDLE_CRS_MAX_ELL)");
  if (!(flags & CURDLE_CRS_TRUSTED) && (!curdle_g1_check_batch || !curdle_g1_check_jac_batch)) return CrsNoDevice("curdle_crs_from_points");
  return Guard([&]() -> int {
    CrsFields f;
    f.ell = ell;
    f.gens = Affines(in->Gs, ell);
    f.gens.resize(ell + proto::N_BLINDERS);
    memcpy(f.gens.data() + ell, in->Hs, proto::N_BLINDERS * sizeof(G1Affine));
    f.H = Point::FromJac(in->H);
    f.Gt = Point::FromJac(in->Gt);
    f.Gu = Point::FromJac(in->Gu);
    memcpy(&f.Gsum, in->Gsum, sizeof(G1Affine));
    memcpy(&f.Hsum, in->Hsum, sizeof(G1Affine));
    if (flags & CURDLE_CRS_TRUSTED) return CrsHandle(f, out, fault);
    // Gs | Hs | Gsum | Hsum staged contiguously for one affine check; H | Gt | Gu, as given, for one Jacobian check
    const size_t n_gens = ell + proto::N_BLINDERS;
    std::vector<G1Affine> affine = f.gens;
    affine.push_back(f.Gsum);
    affine.push_back(f.Hsum);
    uint64_t jac[3 * 18];
    memcpy(jac, in->H, 144);
    memcpy(jac + 18, in->Gt, 144);
    memcpy(jac + 36, in->Gu, 144);
    std::vector<uint8_t> st_affine(affine.size(), 0xff);
    uint8_t st_jac[3] = {0xff, 0xff, 0xff};
    if (int rc = curdle_g1_check_batch(reinterpret_cast<const uint64_t*>(affine.data()), affine.size(), 1, st_affine.data())) return rc;
    if (int rc = curdle_g1_check_jac_batch(jac, 3, 1, st_jac)) return rc;
    std::vector<uint8_t> status(st_affine.begin(), st_affine.begin() + n_gens);  // into wire order
    status.insert(status.end(), st_jac, st_jac + 3);
    status.insert(status.end(), st_affine.begin() + n_gens, st_affine.end());
    return CrsFinishValidated(f, status, /*from_bytes=*/false, out, fault);
  });
}

extern "C" int curdle_crs_from_bytes(const uint8_t* in, size_t len, curdle_crs** out, curdle_crs_fault* fault) {
  if (out) *out = nullptr;
  if (!in || !out) return curdle_set_last_error(CURDLE_EINVAL, "null argument");
  const size_t fixed = proto::N_BLINDERS + kCrsSingles;
  if (len % 48 || len / 48 <= fixed || len / 48 - fixed > CURDLE_CRS_MAX_ELL) {
    char msg[112];
    snprintf(msg, sizeof(msg), "len = %zu is not 48 (ell + 9) for an ell of 1 ... 2^20 (CURDLE_CRS_MAX_ELL)", len);
    return curdle_set_last_error(CURDLE_EINVAL, msg);
  }
  if (!curdle_g1_decompress_batch) return CrsNoDevice("curdle_crs_from_bytes");
  return Guard([&]() -> int {
    const size_t n = len / 48, ell = n - fixed, n_gens = ell + proto::N_BLINDERS;
    std::vector<G1Affine> pts(n);
    std::vector<uint8_t> status(n, 0xff);
    if (int rc = curdle_g1_decompress_batch(in, n, 1, reinterpret_cast<uint64_t*>(pts.data()), status.data())) return rc;
    CrsFields f;  // an invalid record decodes to (0, 0); its status is looked at before any of this is used
    f.ell = ell;
    f.gens.assign(pts.begin(), pts.begin() + n_gens);
    f.H = Point::FromAffine(pts[n_gens]);
    f.Gt = Point::FromAffine(pts[n_gens + 1]);
    f.Gu = Point::FromAffine(pts[n_gens + 2]);
    f.Gsum = pts[n_gens + 3];
    f.Hsum = pts[n_gens + 4];
    return CrsFinishValidated(f, status, /*from_bytes=*/true, out, fault);
  });
}

extern "C" int curdle_crs_export_points(const curdle_crs* crs, uint64_t* Gs, uint64_t* Hs, uint64_t H[18], uint64_t Gt[18],
                                        uint64_t Gu[18], uint64_t Gsum[12], uint64_t Hsum[12]) {
  if (!crs || !Gs || !Hs || !H || !Gt || !Gu || !Gsum || !Hsum) return curdle_set_last_error(CURDLE_EINVAL, "null argument");
  const proto::CRS& k = crs->crs;
  if (!k.Gs.empty()) memcpy(Gs, k.Gs.data(), k.Gs.size() * sizeof(G1Affine));
  if (!k.Hs.empty()) memcpy(Hs, k.Hs.data(), k.Hs.size() * sizeof(G1Affine));
  k.H.Jac(H);
  k.Gt.Jac(Gt);
  k.Gu.Jac(Gu);
  memcpy(Gsum, &k.Gsum, sizeof(G1Affine));
  memcpy(Hsum, &k.Hsum, sizeof(G1Affine));
  return CURDLE_OK;
}

extern "C" int curdle_crs_to_bytes(const curdle_crs* crs, uint8_t* out, size_t cap, size_t* len) {
  if (!crs || !len) return curdle_set_last_error(CURDLE_EINVAL, "null argument");
  const proto::CRS& k = crs->crs;
  const size_t n_gens = k.Gs.size() + k.Hs.size(), need = 48 * (n_gens + kCrsSingles);
  *len = need;
  if (!out) return curdle_set_last_error(CURDLE_EINVAL, "null argument");
  if (cap < need) return curdle_set_last_error(CURDLE_EINVAL, "CRS buffer too small");
  return Guard([&]() {
    alg::CompressAffineBatch(k.Gs.data(), k.Gs.size(), out);
    alg::CompressAffineBatch(k.Hs.data(), k.Hs.size(), out + 48 * k.Gs.size());
    uint8_t* p = out + 48 * n_gens;
    k.H.Compressed(p);
    k.Gt.Compressed(p + 48);
    k.Gu.Compressed(p + 96);
    alg::CompressAffine(k.Gsum, p + 144);
    alg::CompressAffine(k.Hsum, p + 192);
    return CURDLE_OK;
  });
}

extern "C" int curdle_shuffle_permute_commit(const curdle_crs* crs, const uint64_t* Rs, const uint64_t* Ss, size_t ell,
                                             const uint32_t* perm, const uint64_t k[4], curdle_rand* rand,
                                             uint64_t* Ts_out, uint64_t* Us_out, uint64_t M_out[18],
                                             uint64_t rs_m_out[16]) {
  if (!crs || !Rs || !Ss || !perm || !k || !rand || !Ts_out || !Us_out || !M_out || !rs_m_out)
    return curdle_set_last_error(CURDLE_EINVAL, "null argument");
  if (ell != crs->crs.Gs.size()) return curdle_set_last_error(CURDLE_EINVAL, "ell does not match the CRS");
  return Guard([&]() {
    std::vector<uint32_t> pv(perm, perm + ell);
    for (uint32_t v : pv)
      if (v >= ell) throw std::runtime_error("permutation entry out of range");
    proto::ShuffleCommit sc = proto::ShufflePermuteCommit(crs->crs.Gs, crs->crs.Hs, Affines(Rs, ell), Affines(Ss, ell),
                                                          pv, Scalar::FromMont(k), rand->r);
    memcpy(Ts_out, sc.Ts.data(), ell * 96);
    memcpy(Us_out, sc.Us.data(), ell * 96);
    sc.M.Jac(M_out);
    for (int i = 0; i < proto::N_BLINDERS; i++) memcpy(rs_m_out + 4 * i, &sc.rs_m[i].v, 32);
    return CURDLE_OK;
  });
}

// The host's part of curdle_shuffle_permute_commit_ex under CURDLE_SHUFFLE_CONSTANT_TIME (csrc/msm_ct_api.hip owns the entry
// point and the device work): ell against the CRS, the permutation's range (the existing check: a failure reveals only
// that the input was invalid), then the blinders, drawn at the point where the call without flags draws them --
// GetFrs(N_BLINDERS), nothing before it.  Hands out the CRS's Gs and Hs as gnark records.  This, the draw's own code and
// the caller's copies are what lies outside the flag's promise.
int curdle_shuffle_commit_ct_host_part(const curdle_crs* crs, size_t ell, const uint32_t* perm, curdle_rand* rand,
                                       const uint64_t** Gs, const uint64_t** Hs, uint64_t rs_m[16]) {
  if (ell != crs->crs.Gs.size()) return curdle_set_last_error(CURDLE_EINVAL, "ell does not match the CRS");
  return Guard([&]() {
    for (size_t i = 0; i < ell; i++)
      if (perm[i] >= ell) throw std::runtime_error("permutation entry out of range");
    static_assert(proto::N_BLINDERS == 4 && sizeof(Fr) == 32, "rs_m holds four blinders");
    std::vector<Fr> drawn;
    rand->r.GetFrs(proto::N_BLINDERS, drawn);
    memcpy(rs_m, drawn.data(), 128);
    explicit_bzero(drawn.data(), 128);
    *Gs = reinterpret_cast<const uint64_t*>(crs->crs.Gs.data());
    *Hs = reinterpret_cast<const uint64_t*>(crs->crs.Hs.data());
    return CURDLE_OK;
  });
}

extern "C" int curdle_prove(const curdle_crs* crs, const uint64_t* Rs, const uint64_t* Ss, const uint64_t* Ts,
                            const uint64_t* Us, size_t ell, const uint64_t M[18], const uint32_t* perm,
                            const uint64_t k[4], const uint64_t rs_m[16], curdle_rand* rand, uint8_t* proof_out,
                            size_t cap, size_t* proof_len) {
  if (!crs || !Rs || !Ss || !Ts || !Us || !M || !perm || !k || !rs_m || !rand || !proof_len)
    return curdle_set_last_error(CURDLE_EINVAL, "null argument");
  if (ell != crs->crs.Gs.size()) return curdle_set_last_error(CURDLE_EINVAL, "ell does not match the CRS");
  return Guard([&]() {
    std::vector<Scalar> rsm(proto::N_BLINDERS);
    for (int i = 0; i < proto::N_BLINDERS; i++) rsm[i] = Scalar::FromMont(rs_m + 4 * i);
    proto::Proof p = proto::Prove(crs->crs, Affines(Rs, ell), Affines(Ss, ell), Affines(Ts, ell), Affines(Us, ell),
                                  Point::FromJac(M), std::vector<uint32_t>(perm, perm + ell), Scalar::FromMont(k), rsm,
                                  rand->r);
    std::vector<uint8_t> bytes = p.Serialize();
    *proof_len = bytes.size();
    if (!proof_out || cap < bytes.size()) return curdle_set_last_error(CURDLE_EINVAL, "proof buffer too small");
    memcpy(proof_out, bytes.data(), bytes.size());
    return CURDLE_OK;
  });
}

// curdle_prove with a flags word.  Under CURDLE_PROVE_MSM_CONSTANT_TIME the body is curdle_prove's under an
// alg::ConstantTimeMsmScope on this thread (Prove starts no threads): every MSM of the proof goes to the constant-time
// primitive and nothing else differs, so the proof and rand's state afterwards are the unflagged call's.
extern "C" int curdle_prove_ex(const curdle_crs* crs, const uint64_t* Rs, const uint64_t* Ss, const uint64_t* Ts,
                               const uint64_t* Us, size_t ell, const uint64_t M[18], const uint32_t* perm,
                               const uint64_t k[4], const uint64_t rs_m[16], curdle_rand* rand, unsigned flags,
                               uint8_t* proof_out, size_t cap, size_t* proof_len) {
  if (flags & ~CURDLE_PROVE_MSM_CONSTANT_TIME) {
    char msg[64];
    snprintf(msg, sizeof(msg), "unknown flag bits 0x%x", flags & ~CURDLE_PROVE_MSM_CONSTANT_TIME);
    return curdle_set_last_error(CURDLE_EINVAL, msg);
  }
  if (!flags) return curdle_prove(crs, Rs, Ss, Ts, Us, ell, M, perm, k, rs_m, rand, proof_out, cap, proof_len);
  if (!crs || !Rs || !Ss || !Ts || !Us || !M || !perm || !k || !rs_m || !rand || !proof_len)
    return curdle_set_last_error(CURDLE_EINVAL, "null argument");
  if (ell != crs->crs.Gs.size()) return curdle_set_last_error(CURDLE_EINVAL, "ell does not match the CRS");
  if (proto::ProverFoldBasesEnabled())
    return curdle_set_last_error(CURDLE_EINVAL,
                                 "CURDLE_PROVE_MSM_CONSTANT_TIME with PROVER_FOLD_BASES set: that prover multiplies H by a "
                                 "secret inner product on the host");
  if (!alg::ConstantTimeMsmScope::Available())
    return curdle_set_last_error(CURDLE_ENODEV,
                                 "CURDLE_PROVE_MSM_CONSTANT_TIME: the constant-time MSM is not part of this backend");
  alg::ConstantTimeMsmScope scope;
  return curdle_prove(crs, Rs, Ss, Ts, Us, ell, M, perm, k, rs_m, rand, proof_out, cap, proof_len);
}

// Device-backed entry points the constant-time prover and shuffle call.  Weak, as host/algebra.cpp names the
// constant-time MSMs: linked over a backend without them the two calls below fail with CURDLE_ENODEV.
extern "C" int curdle_device_available(void) __attribute__((weak));
extern "C" int curdle_shuffle_permute_commit_ex(const curdle_crs* crs, const uint64_t* Rs, const uint64_t* Ss, size_t ell,
                                                const uint32_t* perm, const uint64_t k[4], curdle_rand* rand, unsigned flags,
                                                uint64_t* Ts_out, uint64_t* Us_out, uint64_t M_out[18],
                                                uint64_t rs_m_out[16]) __attribute__((weak));

static constexpr size_t kProveCtMaxEll = 4096;  // the oblivious gather is quadratic: the shuffle step's cap

// Whether the constant-time prover can run at all, asked before anything is drawn from rand.
static bool ProveCtBackend() {
  return alg::SecretOpsScope::Available() && curdle_device_available && curdle_device_available();
}

// curdle_prove with every operation on a secret off the host's branches and addresses: the body is curdle_prove's under
// an alg::ConstantTimeMsmScope (every MSM to the constant-time primitive) and an alg::SecretOpsScope (the secret scalar
// multiplications as MSMs, the gathers by the permutation through the oblivious gather, no unblinded commitment on the
// host), both on this thread.  Same draws in the same order, same proof bytes.
extern "C" int curdle_prove_ct(const curdle_crs* crs, const uint64_t* Rs, const uint64_t* Ss, const uint64_t* Ts,
                               const uint64_t* Us, size_t ell, const uint64_t M[18], const uint32_t* perm,
                               const uint64_t k[4], const uint64_t rs_m[16], curdle_rand* rand, uint8_t* proof_out,
                               size_t cap, size_t* proof_len) {
  if (!crs || !Rs || !Ss || !Ts || !Us || !M || !perm || !k || !rs_m || !rand || !proof_len)  // proof_out: as curdle_prove
    return curdle_set_last_error(CURDLE_EINVAL, "null argument");
  if (ell != crs->crs.Gs.size()) return curdle_set_last_error(CURDLE_EINVAL, "ell does not match the CRS");
  if (ell > kProveCtMaxEll)
    return curdle_set_last_error(CURDLE_EINVAL, "ell exceeds the 4,096 the constant-time prover supports");
  if (proto::ProverFoldBasesEnabled())
    return curdle_set_last_error(CURDLE_EINVAL,
                                 "CURDLE_PROVE_MSM_CONSTANT_TIME with PROVER_FOLD_BASES set: that prover multiplies H by a "
                                 "secret inner product on the host");
  if (!ProveCtBackend())
    return curdle_set_last_error(CURDLE_ENODEV,
                                 "curdle_prove_ct: the constant-time MSM and the oblivious gather need the device backend and a device");
  alg::ConstantTimeMsmScope msms;
  alg::SecretOpsScope secret_ops;
  return curdle_prove(crs, Rs, Ss, Ts, Us, ell, M, perm, k, rs_m, rand, proof_out, cap, proof_len);
}

// ---------------------------------------------------------------------------------------------------------------------
// curdle_prover_ct: curdle_prove_ct over resident tables.  The handle owns ONE curdle_ct_bases over the CRS's points --
// Gs | Hs | H | Gt | Gu | one all-zero record (the point at infinity, which the same-multiscalar bases pad with) -- made
// once; a Prove runs curdle_prove_ct's body under one more scope, an alg::ResidentBasesScope whose registry is
// {the handle's CRS set, this call's Rs | Ss | Ts | Us} and later {R, S} (curdleproofs.cpp), so every funnel call
// resolves to rows and is one curdle_msm_g1_ct_bases_sets_batch.  The table names are weak, as in host/algebra.cpp.
// ---------------------------------------------------------------------------------------------------------------------
extern "C" int curdle_ct_bases_create(const uint64_t* points, size_t n, unsigned chunk_bits, curdle_ct_bases** out)
    __attribute__((weak));
extern "C" void curdle_ct_bases_free(curdle_ct_bases* b) __attribute__((weak));

struct curdle_prover_ct {
  const curdle_crs* crs = nullptr;
  unsigned c = 0, chunks = 0;    // chunk_bits in force and C = ceil(255 / c)
  std::vector<G1Affine> points;  // what the table holds, in its order
  curdle_ct_bases* table = nullptr;
};

static constexpr size_t kCtBasesMaxRecords = 65536;  // curdle_ct_bases_create's limit on n C

extern "C" int curdle_prover_ct_create(const curdle_crs* crs, unsigned chunk_bits, curdle_prover_ct** out) {
  if (out) *out = nullptr;
  if (!crs || !out) return curdle_set_last_error(CURDLE_EINVAL, "null argument");
  const unsigned c = alg::ResidentBases::ChunkBitsOf(chunk_bits);
  if (c != 8 && c != 16 && c != 32 && c != 64) {
    char msg[96];
    snprintf(msg, sizeof(msg), "chunk_bits = %u is not 8, 16, 32, 64 or 0 (the library's choice)", chunk_bits);
    return curdle_set_last_error(CURDLE_EINVAL, msg);
  }
  const unsigned chunks = (255 + c - 1) / c;
  const proto::CRS& k = crs->crs;
  const size_t n = k.Gs.size() + k.Hs.size() + 4;
  if (n > kCtBasesMaxRecords / chunks) {
    char msg[128];
    snprintf(msg, sizeof(msg), "the CRS is too large for one table: (ell + 8) C = %zu x %u exceeds 65,536 records", n, chunks);
    return curdle_set_last_error(CURDLE_EINVAL, msg);
  }
  if (!alg::ResidentBasesScope::Available() || !ProveCtBackend())
    return curdle_set_last_error(CURDLE_ENODEV,
                                 "curdle_prover_ct_create: the constant-time base tables and prover need the device backend and a device");
  return Guard([&]() -> int {
    std::unique_ptr<curdle_prover_ct> p(new curdle_prover_ct());
    p->crs = crs;
    p->c = c;
    p->chunks = chunks;
    p->points = k.Gs;
    p->points.insert(p->points.end(), k.Hs.begin(), k.Hs.end());
    p->points.push_back(k.H.Affine());
    p->points.push_back(k.Gt.Affine());
    p->points.push_back(k.Gu.Affine());
    G1Affine zero;
    memset(&zero, 0, sizeof(zero));
    p->points.push_back(zero);
    if (int rc = curdle_ct_bases_create(reinterpret_cast<const uint64_t*>(p->points.data()), p->points.size(), c, &p->table)) return rc;
    *out = p.release();
    return CURDLE_OK;
  });
}

extern "C" void curdle_prover_ct_free(curdle_prover_ct* p) {
  if (!p) return;
  if (p->table && curdle_ct_bases_free) curdle_ct_bases_free(p->table);
  delete p;
}

extern "C" int curdle_prover_ct_prove(curdle_prover_ct* p, const uint64_t* Rs, const uint64_t* Ss, const uint64_t* Ts,
                                      const uint64_t* Us, size_t ell, const uint64_t M[18], const uint32_t* perm,
                                      const uint64_t k[4], const uint64_t rs_m[16], curdle_rand* rand, uint8_t* proof_out,
                                      size_t cap, size_t* proof_len) {
  // curdle_prove_ct's refusals, in its order
  if (!p || !Rs || !Ss || !Ts || !Us || !M || !perm || !k || !rs_m || !rand || !proof_len)
    return curdle_set_last_error(CURDLE_EINVAL, "null argument");
  const curdle_crs* crs = p->crs;
  if (ell != crs->crs.Gs.size()) return curdle_set_last_error(CURDLE_EINVAL, "ell does not match the CRS");
  if (ell > kProveCtMaxEll)
    return curdle_set_last_error(CURDLE_EINVAL, "ell exceeds the 4,096 the constant-time prover supports");
  if (proto::ProverFoldBasesEnabled())
    return curdle_set_last_error(CURDLE_EINVAL,
                                 "CURDLE_PROVE_MSM_CONSTANT_TIME with PROVER_FOLD_BASES set: that prover multiplies H by a "
                                 "secret inner product on the host");
  if (!ProveCtBackend())
    return curdle_set_last_error(CURDLE_ENODEV,
                                 "curdle_prove_ct: the constant-time MSM and the oblivious gather need the device backend and a device");
  // Before anything is drawn from rand: this call's registry.  The CRS set is the handle's, shared and read-only; the
  // instance vectors are this call's set, freed with the registry on every way out.  A public decision on ell: instance
  // vectors beyond one table (4 ell C > 65,536) leave the registry empty and declining, and the call runs exactly as
  // curdle_prove_ct.
  return Guard([&]() -> int {
    alg::ResidentBases registry(p->c);
    if (4 * ell > kCtBasesMaxRecords / p->chunks) {
      registry.Decline();
    } else {
      registry.AddShared(p->table, p->points);
      std::vector<G1Affine> inst(4 * ell);
      const uint64_t* parts[4] = {Rs, Ss, Ts, Us};
      for (int i = 0; i < 4; i++)
        if (ell) memcpy(inst.data() + i * ell, parts[i], ell * 96);
      registry.Add(inst);
    }
    alg::ConstantTimeMsmScope msms;
    alg::SecretOpsScope secret_ops;
    alg::ResidentBasesScope resident(registry);
    return curdle_prove(crs, Rs, Ss, Ts, Us, ell, M, perm, k, rs_m, rand, proof_out, cap, proof_len);
  });
}

// ---------------------------------------------------------------------------------------------------------------------
// curdle_prove_batch: k Proves over one CRS at one ell in lockstep (alg::Lockstep, algebra.h).  Every member runs
// curdle_prove's body on a thread of its own under a LockstepScope -- under the flag also under the two constant-time
// scopes, which makes it curdle_prove_ct's -- and the members' funnel calls meet at each step and go to the device as
// ONE coalesced call.  The results a member gets back are those of its own call, so its proof, its length and its
// rand's state afterwards are the single call's.
// ---------------------------------------------------------------------------------------------------------------------
static std::atomic<unsigned long long> g_prove_batch_stat[4];  // calls | members | groups | coalesced device calls

static size_t ProveBatchGroup() {
  const long long v = knobs::get(knobs::PROVE_BATCH_GROUP);
  return v >= 1 && v <= 64 ? (size_t)v : 64;
}

// The call's verdict over its members' codes.  A member's own failure is CURDLE_EINVAL (Guard: a structural error of the
// protocol) and leaves the call CURDLE_OK.  What fails the call, each with its own text: a member thread that could not
// be started, a step at which the members' requests disagreed (the library's fault, not the device's: it reaches the
// members as an MsmError), and a failed device call.
static int BatchVerdict(const int* status, size_t k, const char* who, const alg::LockstepRun& run) {
  char msg[200];
  if (run.not_started) {
    snprintf(msg, sizeof(msg), "%s: %zu member thread(s) could not be started", who, run.not_started);
    return curdle_set_last_error(CURDLE_ENOMEM, msg);
  }
  for (size_t i = 0; i < k; i++)
    if (status[i] != CURDLE_OK && status[i] != CURDLE_EINVAL) {
      if (run.disagreements)
        snprintf(msg, sizeof(msg), "%s: the members' requests disagreed at %llu step(s) (funnel, shapes or switches): not a device failure",
                 who, run.disagreements);
      else
        snprintf(msg, sizeof(msg), "%s: a device call failed (member %zu: code %d)", who, i, status[i]);
      return curdle_set_last_error(status[i], msg);
    }
  return CURDLE_OK;
}

static void CountProveBatch(size_t k, const alg::LockstepRun& run) {
  g_prove_batch_stat[0].fetch_add(1, std::memory_order_relaxed);
  g_prove_batch_stat[1].fetch_add(k, std::memory_order_relaxed);
  g_prove_batch_stat[2].fetch_add(run.groups, std::memory_order_relaxed);
  g_prove_batch_stat[3].fetch_add(run.device_calls, std::memory_order_relaxed);
}

// Two members drawing from one generator on two threads would be a race, and no single call's draws.
static bool DistinctRands(curdle_rand* const* rands, size_t k) {
  std::vector<const curdle_rand*> v(rands, rands + k);
  std::sort(v.begin(), v.end());
  return std::adjacent_find(v.begin(), v.end()) == v.end();
}

extern "C" int curdle_prove_batch(const curdle_crs* crs, size_t k, size_t ell, const uint64_t* const* Rs,
                                  const uint64_t* const* Ss, const uint64_t* const* Ts, const uint64_t* const* Us,
                                  const uint64_t* Ms, const uint32_t* const* perms, const uint64_t* ks, const uint64_t* rs_ms,
                                  curdle_rand* const* rands, unsigned flags, uint8_t* proofs_out, size_t stride,
                                  size_t* proof_lens, int* status) {
  if (flags & ~CURDLE_PROVE_BATCH_CONSTANT_TIME) {
    char msg[64];
    snprintf(msg, sizeof(msg), "unknown flag bits 0x%x", flags & ~CURDLE_PROVE_BATCH_CONSTANT_TIME);
    return curdle_set_last_error(CURDLE_EINVAL, msg);
  }
  if (!crs || (k && (!Rs || !Ss || !Ts || !Us || !Ms || !perms || !ks || !rs_ms || !rands || !proofs_out || !proof_lens || !status)))
    return curdle_set_last_error(CURDLE_EINVAL, "null argument");
  for (size_t i = 0; i < k; i++)
    if (!Rs[i] || !Ss[i] || !Ts[i] || !Us[i] || !perms[i] || !rands[i])
      return curdle_set_last_error(CURDLE_EINVAL, "null argument in batch member");
  if (k && !DistinctRands(rands, k)) return curdle_set_last_error(CURDLE_EINVAL, "two members share one rand");
  if (ell != crs->crs.Gs.size()) return curdle_set_last_error(CURDLE_EINVAL, "ell does not match the CRS");
  const bool ct = flags & CURDLE_PROVE_BATCH_CONSTANT_TIME;
  if (ct) {  // curdle_prove_ct's refusals, in its order
    if (ell > kProveCtMaxEll)
      return curdle_set_last_error(CURDLE_EINVAL, "ell exceeds the 4,096 the constant-time prover supports");
    if (proto::ProverFoldBasesEnabled())
      return curdle_set_last_error(CURDLE_EINVAL,
                                   "CURDLE_PROVE_BATCH_CONSTANT_TIME with PROVER_FOLD_BASES set: that prover multiplies H by a "
                                   "secret inner product on the host");
    if (k && !ProveCtBackend())
      return curdle_set_last_error(CURDLE_ENODEV,
                                   "curdle_prove_batch: the constant-time MSM and the oblivious gather need the device backend and a device");
  }
  if (k == 0) return CURDLE_OK;
  const alg::LockstepRun run = alg::RunInLockstep(
      k, ProveBatchGroup(), ct,
      [&](size_t i) {
        proof_lens[i] = 0;
        status[i] = curdle_prove(crs, Rs[i], Ss[i], Ts[i], Us[i], ell, Ms + 18 * i, perms[i], ks + 4 * i, rs_ms + 16 * i, rands[i],
                                 proofs_out + stride * i, stride, &proof_lens[i]);
        if (status[i] != CURDLE_OK) proof_lens[i] = 0;
      },
      [&](size_t i) {
        proof_lens[i] = 0;
        status[i] = CURDLE_ENOMEM;
      });
  CountProveBatch(k, run);
  return BatchVerdict(status, k, "curdle_prove_batch", run);
}

extern "C" int curdle_stat_prove_batch(unsigned long long out[4]) {
  if (!out) return curdle_set_last_error(CURDLE_EINVAL, "null argument");
  for (int i = 0; i < 4; i++) out[i] = g_prove_batch_stat[i].load(std::memory_order_relaxed);
  return CURDLE_OK;
}

extern "C" int curdle_stat_host_point_mul(unsigned long long* out) {
  if (!out) return curdle_set_last_error(CURDLE_EINVAL, "null argument");
  *out = alg::PointMulCalls();
  return CURDLE_OK;
}

extern "C" int curdle_stat_alg_msm(unsigned long long out[4]) {
  if (!out) return curdle_set_last_error(CURDLE_EINVAL, "null argument");
  alg::ReadMsmCounters(out);
  return CURDLE_OK;
}

extern "C" int curdle_verify(const curdle_crs* crs, const uint8_t* proof, size_t proof_len, const uint64_t* Rs,
                             const uint64_t* Ss, const uint64_t* Ts, const uint64_t* Us, size_t ell,
                             const uint64_t M[18], curdle_rand* rand, int* ok) {
  if (!crs || !proof || !Rs || !Ss || !Ts || !Us || !M || !rand || !ok)
    return curdle_set_last_error(CURDLE_EINVAL, "null argument");
  *ok = 0;
  if (ell != crs->crs.Gs.size()) return curdle_set_last_error(CURDLE_EINVAL, "ell does not match the CRS");
  return Guard([&]() {
    // gnark's Decoder checks curve and subgroup membership of every point (curdleproof.go:322).
    // The subgroup half of that runs on the GPU while the host verifies; its verdict is
    // collected before anything is reported.
    proto::PointDecoder dec(/*subgroup_check=*/true);
    const Point Mp = Point::FromJac(M);
    bool accept;
    if (proto::CanVerifyWhileDecoding()) {
      // one pass over the wire format: the records go to the GPU, the proof comes back with its
      // points pending, and the WHOLE host part (transcript, challenge algebra) runs from the
      // bytes while the decoding kernel takes the square roots
      proto::Reader scan(proof, proof_len, true);
      scan.collect = &dec;
      const proto::Proof p = proto::Proof::ScanLazy(scan);
      dec.Start();
      proto::DecodedInstance given{Affines(Rs, ell), Affines(Ss, ell), Affines(Ts, ell), Affines(Us, ell)};
      proto::VerifyPrelude pre;
      proto::StartVerify(pre, given.Rs, given.Ss, given.Ts, given.Us, Mp);
      accept = proto::VerifyWhileDecoding(
          pre, p, crs->crs, Mp, dec,
          [&](proto::DecodedInstance& inst) {
            G1Affine a;
            for (size_t i = 0; i < dec.size(); i++)
              if (!dec.GetAffine(i, &a)) throw std::runtime_error("decoding proof: invalid point");
            inst = std::move(given);
          },
          rand->r);
    } else {
      proto::Proof::ScanAndStart(proof, proof_len, dec);  // the GPU takes the square roots ...
      const std::vector<G1Affine> R = Affines(Rs, ell), S = Affines(Ss, ell), T = Affines(Ts, ell), U = Affines(Us, ell);
      proto::VerifyPrelude pre;
      proto::StartVerify(pre, R, S, T, U, Mp);            // ... while the host absorbs the instance and draws `as`
      proto::Proof p = proto::Proof::FromStarted(proof, proof_len, dec);
      accept = proto::VerifyStarted(pre, p, crs->crs, R, S, T, U, Mp, rand->r);
    }
    if (!dec.Finish()) throw std::runtime_error("decoding proof: invalid point (not in the prime-order subgroup)");
    *ok = accept ? 1 : 0;
    return CURDLE_OK;
  });
}

extern "C" int curdle_proof_from_bytes(const uint8_t* proof, size_t proof_len, curdle_proof** out) {
  if (!proof || !out) return curdle_set_last_error(CURDLE_EINVAL, "null argument");
  *out = nullptr;
  return Guard([&]() {
    curdle_proof* h = new curdle_proof();
    try {
      h->p = proto::Proof::FromBytes(proof, proof_len, /*subgroup_check=*/true);
    } catch (...) {
      delete h;
      throw;
    }
    *out = h;
    return CURDLE_OK;
  });
}
extern "C" void curdle_proof_free(curdle_proof* p) { delete p; }

extern "C" int curdle_verify_proof(const curdle_crs* crs, const curdle_proof* proof, const uint64_t* Rs, const uint64_t* Ss,
                                   const uint64_t* Ts, const uint64_t* Us, size_t ell, const uint64_t M[18],
                                   curdle_rand* rand, int* ok) {
  if (!crs || !proof || !Rs || !Ss || !Ts || !Us || !M || !rand || !ok)
    return curdle_set_last_error(CURDLE_EINVAL, "null argument");
  *ok = 0;
  if (ell != crs->crs.Gs.size()) return curdle_set_last_error(CURDLE_EINVAL, "ell does not match the CRS");
  return Guard([&]() {
    bool accept = proto::Verify(proof->p, crs->crs, Affines(Rs, ell), Affines(Ss, ell), Affines(Ts, ell), Affines(Us, ell),
                                Point::FromJac(M), rand->r);
    *ok = accept ? 1 : 0;
    return CURDLE_OK;
  });
}

// Where the verifier's accumulator lives: 1 (default) on the device, 0 on the host mirror.
extern "C" int curdle_verify_set_device_acc(int on) { return proto::SetDeviceAccumulator(on); }

// The accumulated (base, scalar) list of one verification, before the final MSM, from the host
// mirror (device = 0) or from the device accumulator (device = 1), and the accept bit: what
// the parity test of the two accumulators compares (tests/test_device_accumulator.py).
extern "C" int curdle_verify_export_accumulator(const curdle_crs* crs, const curdle_proof* proof, const uint64_t* Rs,
                                                const uint64_t* Ss, const uint64_t* Ts, const uint64_t* Us, size_t ell,
                                                const uint64_t M[18], curdle_rand* rand, int device, uint64_t* points,
                                                uint64_t* scalars, size_t cap, size_t* n_out, int* ok) {
  if (!crs || !proof || !Rs || !Ss || !Ts || !Us || !M || !rand || !n_out || !ok)
    return curdle_set_last_error(CURDLE_EINVAL, "null argument");
  if (ell != crs->crs.Gs.size()) return curdle_set_last_error(CURDLE_EINVAL, "ell does not match the CRS");
  return Guard([&]() {
    const std::vector<G1Affine> R = Affines(Rs, ell), S = Affines(Ss, ell), T = Affines(Ts, ell), U = Affines(Us, ell);
    std::vector<G1Affine> bases;
    std::vector<Scalar> sc;
    bool accept = false;
    if (device) {
      proto::DeviceSink sink(crs->crs, R, S, T, U);
      if (proto::VerifyWithSink(proof->p, crs->crs, R, S, T, U, Point::FromJac(M), rand->r, sink))
        accept = sink.VerifyAndExport(&bases, &sc);
    } else {
      msmaccumulator::MsmAccumulator acc;
      if (proto::VerifyInto(proof->p, crs->crs, R, S, T, U, Point::FromJac(M), rand->r, acc)) {
        bases = acc.Bases();
        sc.resize(acc.Scalars().size());
        for (size_t i = 0; i < sc.size(); i++) sc[i].v = acc.Scalars()[i];
        msmaccumulator::Status st = acc.Verify(&accept);
        if (!st.ok) throw alg::MsmError("verifying msm accumulator: " + st.err, st.rc ? st.rc : CURDLE_EHIP);
      }
    }
    *n_out = bases.size();
    *ok = accept ? 1 : 0;
    if (bases.size() > cap || (bases.size() && (!points || !scalars)))
      return curdle_set_last_error(CURDLE_EINVAL, "export buffers too small");
    if (!bases.empty()) {
      memcpy(points, bases.data(), bases.size() * 96);
      memcpy(scalars, sc.data(), sc.size() * 32);
    }
    return CURDLE_OK;
  });
}

// A batch over SEVERAL devices (curdle_init_devices): contiguous shards of the k proofs, one
// per context, each verified by its own group of host threads that select the shard's device
// first -- BASELINE config 5 (many independent verifications) is replicas: no data moves
// between devices, and the accept bits are exactly those of the single-device call.  run(lo,
// hi, rand, threads) verifies proofs [lo, hi) on the calling thread's device.
template <class Run>
static std::vector<int> ShardOverDevices(size_t k, common::Rand& rand, int nthreads, Run run) {
  const int D = curdle_device_count();
  if (D <= 1 || k < (size_t)(2 * D)) return run((size_t)0, k, rand, nthreads);
  if (nthreads < 1) nthreads = 1;
  std::vector<uint64_t> seeds((size_t)D);
  for (auto& sd : seeds) {  // each shard its own verifier randomness, drawn from the caller's
    Fr f;
    rand.GetFr(f);
    sd = (uint64_t)f.l[0] | ((uint64_t)f.l[1] << 32);
  }
  const int per = nthreads / D > 2 ? nthreads / D : 2;
  std::vector<std::vector<int>> res((size_t)D);
  std::vector<std::exception_ptr> errs((size_t)D);
  std::vector<std::thread> th;
  for (int d = 0; d < D; d++)
    th.emplace_back([&, d] {
      try {
        if (curdle_set_device(d) != CURDLE_OK) throw std::runtime_error("selecting a device for a batch shard");
        const size_t lo = k * (size_t)d / (size_t)D, hi = k * (size_t)(d + 1) / (size_t)D;
        common::Rand r(seeds[(size_t)d]);
        res[(size_t)d] = run(lo, hi, r, per);
      } catch (...) {
        errs[(size_t)d] = std::current_exception();
      }
    });
  for (auto& t : th) t.join();
  for (auto& e : errs)
    if (e) std::rethrow_exception(e);
  std::vector<int> all;
  all.reserve(k);
  for (auto& r : res) all.insert(all.end(), r.begin(), r.end());
  return all;
}

extern "C" int curdle_verify_batch(const curdle_crs* crs, size_t k, const uint8_t* const* proofs, const size_t* proof_lens,
                                   const uint64_t* const* Rs, const uint64_t* const* Ss, const uint64_t* const* Ts,
                                   const uint64_t* const* Us, size_t ell, const uint64_t* Ms, curdle_rand* rand,
                                   int nthreads, int* oks) {
  if (!crs || !rand || !oks || (k && (!proofs || !proof_lens || !Rs || !Ss || !Ts || !Us || !Ms)))
    return curdle_set_last_error(CURDLE_EINVAL, "null argument");
  if (ell != crs->crs.Gs.size()) return curdle_set_last_error(CURDLE_EINVAL, "ell does not match the CRS");
  return Guard([&]() {
    std::vector<proto::BatchItem> items(k);
    for (size_t i = 0; i < k; i++) {
      if (!proofs[i] || !Rs[i] || !Ss[i] || !Ts[i] || !Us[i]) throw std::runtime_error("null argument in batch item");
      items[i] = proto::BatchItem{proofs[i],
                                  proof_lens[i],
                                  reinterpret_cast<const G1Affine*>(Rs[i]),
                                  reinterpret_cast<const G1Affine*>(Ss[i]),
                                  reinterpret_cast<const G1Affine*>(Ts[i]),
                                  reinterpret_cast<const G1Affine*>(Us[i]),
                                  ell,
                                  Ms + 18 * i};
    }
    std::vector<int> res = ShardOverDevices(k, rand->r, nthreads, [&](size_t lo, size_t hi, common::Rand& r, int threads) {
      if (lo == 0 && hi == k) return proto::VerifyBatch(crs->crs, items, r, threads);
      std::vector<proto::BatchItem> shard(items.begin() + lo, items.begin() + hi);
      return proto::VerifyBatch(crs->crs, shard, r, threads);
    });
    for (size_t i = 0; i < k; i++) oks[i] = res[i];
    return CURDLE_OK;
  });
}

// curdle_verify_batch_checked behind its argument checks (csrc/check_api.hip owns the entry point and the check).
int curdle_verify_batch_checked_with(const curdle_crs* crs, size_t k, const uint8_t* const* proofs, const size_t* proof_lens,
                                     const uint64_t* const* Rs, const uint64_t* const* Ss, const uint64_t* const* Ts,
                                     const uint64_t* const* Us, size_t ell, const uint64_t* Ms, curdle_rand* rand, int nthreads,
                                     int* oks, curdle_point_fault* faults, const proto::ChunkCheckFn& check,
                                     unsigned long long stats[2]) {
  const int rc = Guard([&]() {
    std::vector<curdle_point_fault> found(k);
    std::vector<proto::BatchItem> items(k);
    for (size_t i = 0; i < k; i++) {
      if (!proofs[i] || !Rs[i] || !Ss[i] || !Ts[i] || !Us[i]) throw std::runtime_error("null argument in batch item");
      items[i] = proto::BatchItem{proofs[i],
                                  proof_lens[i],
                                  reinterpret_cast<const G1Affine*>(Rs[i]),
                                  reinterpret_cast<const G1Affine*>(Ss[i]),
                                  reinterpret_cast<const G1Affine*>(Ts[i]),
                                  reinterpret_cast<const G1Affine*>(Us[i]),
                                  ell,
                                  Ms + 18 * i};
    }
    std::atomic<unsigned long long> chunks(0);
    std::vector<int> res = ShardOverDevices(k, rand->r, nthreads, [&](size_t lo, size_t hi, common::Rand& r, int threads) {
      std::vector<proto::BatchItem> shard(items.begin() + lo, items.begin() + hi);
      size_t done = 0;
      std::vector<int> bits = proto::VerifyBatchChecked(crs->crs, shard, r, threads, check, found.data() + lo, &done);
      chunks.fetch_add(done);
      return bits;
    });
    unsigned long long rejected = 0;
    for (size_t i = 0; i < k; i++) {
      oks[i] = res[i];
      if (found[i].code > CURDLE_DECODE_INFINITY) rejected++;
      if (faults) faults[i] = found[i];
    }
    stats[0] += rejected;
    stats[1] += chunks.load();
    return CURDLE_OK;
  });
  if (rc != CURDLE_OK)
    for (size_t i = 0; i < k; i++) {
      oks[i] = 0;
      if (faults) faults[i] = curdle_point_fault{0xff, 0, 0, 0};
    }
  return rc;
}

// ---- whisk package (whisk/whisk.go) ----
static std::vector<whisk::WhiskTracker> Trackers(const uint8_t* p, size_t n) {
  std::vector<whisk::WhiskTracker> v(n);
  static_assert(sizeof(whisk::WhiskTracker) == 96, "tracker layout");
  if (n) memcpy(v.data(), p, n * 96);
  return v;
}

extern "C" int curdle_whisk_is_valid_shuffle_proof(const curdle_crs* crs, const uint8_t* pre_trackers,
                                                   const uint8_t* post_trackers, size_t n_pre, size_t n_post,
                                                   const uint8_t* proof, curdle_rand* rand, int* ok) {
  if (!crs || !proof || !rand || !ok || (n_pre && !pre_trackers) || (n_post && !post_trackers))
    return curdle_set_last_error(CURDLE_EINVAL, "null argument");
  *ok = 0;
  return Guard([&]() {
    *ok = whisk::IsValidWhiskShuffleProof(crs->crs, Trackers(pre_trackers, n_pre), Trackers(post_trackers, n_post), proof,
                                          rand->r)
              ? 1
              : 0;
    return CURDLE_OK;
  });
}

extern "C" int curdle_whisk_is_valid_shuffle_proof_batch(const curdle_crs* crs, size_t k, const uint8_t* const* pre_trackers,
                                                         const uint8_t* const* post_trackers, size_t n,
                                                         const uint8_t* const* proofs, curdle_rand* rand, int nthreads,
                                                         int* oks) {
  if (!crs || !rand || !oks || (k && (!pre_trackers || !post_trackers || !proofs)))
    return curdle_set_last_error(CURDLE_EINVAL, "null argument");
  return Guard([&]() {
    std::vector<whisk::ShuffleBatchItem> items(k);
    for (size_t i = 0; i < k; i++) {
      if (!pre_trackers[i] || !post_trackers[i] || !proofs[i]) throw std::runtime_error("null argument in batch item");
      items[i] = whisk::ShuffleBatchItem{reinterpret_cast<const whisk::WhiskTracker*>(pre_trackers[i]),
                                         reinterpret_cast<const whisk::WhiskTracker*>(post_trackers[i]), n, proofs[i]};
    }
    std::vector<int> res = ShardOverDevices(k, rand->r, nthreads, [&](size_t lo, size_t hi, common::Rand& r, int threads) {
      if (lo == 0 && hi == k) return whisk::IsValidWhiskShuffleProofBatch(crs->crs, items, r, threads);
      std::vector<whisk::ShuffleBatchItem> shard(items.begin() + lo, items.begin() + hi);
      return whisk::IsValidWhiskShuffleProofBatch(crs->crs, shard, r, threads);
    });
    for (size_t i = 0; i < k; i++) oks[i] = res[i];
    return CURDLE_OK;
  });
}

extern "C" int curdle_whisk_generate_shuffle_proof(const curdle_crs* crs, const uint8_t* pre_trackers, size_t n,
                                                   curdle_rand* rand, uint8_t* post_trackers_out, uint8_t* proof_out) {
  if (!crs || !pre_trackers || !rand || !post_trackers_out || !proof_out)
    return curdle_set_last_error(CURDLE_EINVAL, "null argument");
  return Guard([&]() {
    std::vector<whisk::WhiskTracker> post = whisk::GenerateWhiskShuffleProof(crs->crs, Trackers(pre_trackers, n), rand->r, proof_out);
    memcpy(post_trackers_out, post.data(), post.size() * 96);
    return CURDLE_OK;
  });
}

// GenerateWhiskShuffleProof with the secrets -- the permutation, k, the blinders -- kept off the host's branches and
// addresses: the draws and their order are the unflagged call's, the decode is public, the shuffle step runs under
// CURDLE_SHUFFLE_CONSTANT_TIME and the proof through curdle_prove_ct.  This call's own copies of k, the permutation and
// rs_m are overwritten on every way out.
// `prover`: null for curdle_prove_ct, or the handle whose curdle_prover_ct_prove makes the proof; nothing else differs.
static int WhiskShuffleProofCt(const curdle_crs* crs, curdle_prover_ct* prover, const uint8_t* pre_trackers, size_t n,
                               curdle_rand* rand, uint8_t* post_trackers_out, uint8_t* proof_out) {
  if (!crs || !pre_trackers || !rand || !post_trackers_out || !proof_out)
    return curdle_set_last_error(CURDLE_EINVAL, "null argument");
  if (!curdle_shuffle_permute_commit_ex || !ProveCtBackend())
    return curdle_set_last_error(CURDLE_ENODEV,
                                 "curdle_whisk_generate_shuffle_proof_ct: the constant-time shuffle step and prover need the "
                                 "device backend and a device");
  struct Secrets {
    std::vector<uint32_t> permutation;
    uint64_t k[4] = {0, 0, 0, 0};
    uint64_t rs_m[16] = {};
    ~Secrets() {
      if (!permutation.empty()) explicit_bzero(permutation.data(), permutation.size() * sizeof(uint32_t));
      explicit_bzero(k, sizeof(k));
      explicit_bzero(rs_m, sizeof(rs_m));
    }
  } s;
  return Guard([&]() -> int {
    rand->r.GeneratePermutation(whisk::ELL, s.permutation);  // whisk.go:64
    static_assert(sizeof(Fr) == sizeof(s.k), "k is one fr.Element");
    Fr drawn;
    rand->r.GetFr(drawn);                                    // :68
    memcpy(s.k, &drawn, sizeof(s.k));
    explicit_bzero(&drawn, sizeof(drawn));
    whisk::CheckShuffleSize(n);
    std::vector<G1Affine> Rs, Ss;
    whisk::DecodeTrackers(Trackers(pre_trackers, n), &Rs, &Ss);
    std::vector<G1Affine> Ts(n), Us(n);
    uint64_t M[18];
    const uint64_t* R64 = reinterpret_cast<const uint64_t*>(Rs.data());
    const uint64_t* S64 = reinterpret_cast<const uint64_t*>(Ss.data());
    uint64_t* T64 = reinterpret_cast<uint64_t*>(Ts.data());
    uint64_t* U64 = reinterpret_cast<uint64_t*>(Us.data());
    int rc = curdle_shuffle_permute_commit_ex(crs, R64, S64, n, s.permutation.data(), s.k, rand, CURDLE_SHUFFLE_CONSTANT_TIME,
                                              T64, U64, M, s.rs_m);  // :83
    if (rc != CURDLE_OK) return rc;
    std::vector<uint8_t> body(whisk::WHISK_SHUFFLE_PROOF_SIZE);
    size_t body_len = 0;
    rc = prover ? curdle_prover_ct_prove(prover, R64, S64, T64, U64, n, M, s.permutation.data(), s.k, s.rs_m, rand, body.data(),
                                         body.size(), &body_len)
                : curdle_prove_ct(crs, R64, S64, T64, U64, n, M, s.permutation.data(), s.k, s.rs_m, rand, body.data(), body.size(),
                                  &body_len);  // :88
    if (rc != CURDLE_OK) return rc;
    whisk::SerializeShuffleProof(Point::FromJac(M), body.data(), body_len, proof_out);
    for (size_t i = 0; i < n; i++) {  // :109-112
      const whisk::WhiskTracker t = whisk::NewWhiskTracker(Ts[i], Us[i]);
      memcpy(post_trackers_out + 96 * i, &t, 96);
    }
    return CURDLE_OK;
  });
}

extern "C" int curdle_whisk_generate_shuffle_proof_ct(const curdle_crs* crs, const uint8_t* pre_trackers, size_t n,
                                                      curdle_rand* rand, uint8_t* post_trackers_out, uint8_t* proof_out) {
  return WhiskShuffleProofCt(crs, nullptr, pre_trackers, n, rand, post_trackers_out, proof_out);
}

// curdle_whisk_generate_shuffle_proof_ct with its Prove through the handle; the shuffle step is unchanged.
extern "C" int curdle_prover_ct_whisk_shuffle_proof(curdle_prover_ct* p, const uint8_t* pre_trackers, size_t n, curdle_rand* rand,
                                                    uint8_t* post_trackers_out, uint8_t* proof_out) {
  return WhiskShuffleProofCt(p ? p->crs : nullptr, p, pre_trackers, n, rand, post_trackers_out, proof_out);
}

extern "C" int curdle_stat_alg_msm_resident(unsigned long long out[4]) {
  if (!out) return curdle_set_last_error(CURDLE_EINVAL, "null argument");
  alg::ReadResidentCounters(out);
  return CURDLE_OK;
}

// curdle_whisk_generate_shuffle_proof (flags = 0) or curdle_whisk_generate_shuffle_proof_ct (under the flag) for k
// pre-tracker arrays of one n, in lockstep: whisk::GenerateWhiskShuffleProofBatch.
extern "C" int curdle_whisk_generate_shuffle_proof_batch(const curdle_crs* crs, size_t k, const uint8_t* const* pre_trackers,
                                                         size_t n, curdle_rand* const* rands, unsigned flags,
                                                         uint8_t* post_trackers_out, uint8_t* proofs_out, int* status) {
  if (flags & ~CURDLE_PROVE_BATCH_CONSTANT_TIME) {
    char msg[64];
    snprintf(msg, sizeof(msg), "unknown flag bits 0x%x", flags & ~CURDLE_PROVE_BATCH_CONSTANT_TIME);
    return curdle_set_last_error(CURDLE_EINVAL, msg);
  }
  if (!crs || (k && (!pre_trackers || !rands || !post_trackers_out || !proofs_out || !status)))
    return curdle_set_last_error(CURDLE_EINVAL, "null argument");
  for (size_t i = 0; i < k; i++)
    if (!pre_trackers[i] || !rands[i]) return curdle_set_last_error(CURDLE_EINVAL, "null argument in batch member");
  if (k && !DistinctRands(rands, k)) return curdle_set_last_error(CURDLE_EINVAL, "two members share one rand");
  const bool ct = flags & CURDLE_PROVE_BATCH_CONSTANT_TIME;
  if (ct && k && !ProveCtBackend())
    return curdle_set_last_error(CURDLE_ENODEV,
                                 "curdle_whisk_generate_shuffle_proof_batch: the constant-time shuffle step and prover need the "
                                 "device backend and a device");
  if (k == 0) return CURDLE_OK;
  return Guard([&]() -> int {
    std::vector<const whisk::WhiskTracker*> pre(k);
    std::vector<common::Rand*> rs(k);
    for (size_t i = 0; i < k; i++) {
      pre[i] = reinterpret_cast<const whisk::WhiskTracker*>(pre_trackers[i]);
      rs[i] = &rands[i]->r;
    }
    alg::LockstepRun run;
    std::vector<std::string> what;
    const std::vector<int> st = whisk::GenerateWhiskShuffleProofBatch(
        crs->crs, pre, n, rs, ct, ProveBatchGroup(), reinterpret_cast<whisk::WhiskTracker*>(post_trackers_out), proofs_out, &run, &what);
    for (size_t i = 0; i < k; i++) status[i] = st[i];
    CountProveBatch(k, run);
    if (int rc = BatchVerdict(status, k, "curdle_whisk_generate_shuffle_proof_batch", run)) return rc;
    for (size_t i = 0; i < k; i++)  // the call is CURDLE_OK; curdle_last_error still says why the first failed member failed
      if (status[i] != CURDLE_OK) {
        (void)curdle_set_last_error(status[i], what[i].c_str());
        break;
      }
    return CURDLE_OK;
  });
}

extern "C" int curdle_whisk_is_valid_tracker_proof(const uint8_t* tracker, const uint8_t* k_commitment, const uint8_t* proof,
                                                   int* ok) {
  if (!tracker || !k_commitment || !proof || !ok) return curdle_set_last_error(CURDLE_EINVAL, "null argument");
  *ok = 0;
  return Guard([&]() {
    whisk::WhiskTracker t;
    memcpy(&t, tracker, 96);
    *ok = whisk::IsValidWhiskTrackerProof(t, k_commitment, proof) ? 1 : 0;
    return CURDLE_OK;
  });
}

extern "C" int curdle_whisk_generate_tracker_proof(const uint8_t* tracker, const uint64_t k[4], curdle_rand* rand,
                                                   uint8_t* proof_out) {
  if (!tracker || !k || !rand || !proof_out) return curdle_set_last_error(CURDLE_EINVAL, "null argument");
  return Guard([&]() {
    whisk::WhiskTracker t;
    memcpy(&t, tracker, 96);
    whisk::GenerateWhiskTrackerProof(t, Scalar::FromMont(k), rand->r, proof_out);
    return CURDLE_OK;
  });
}

extern "C" int curdle_whisk_is_own_tracker(const uint8_t* tracker, const uint64_t k[4], int* owned) {
  if (!tracker || !k || !owned) return curdle_set_last_error(CURDLE_EINVAL, "null argument");
  *owned = 0;
  return Guard([&]() {
    whisk::WhiskTracker t;
    memcpy(&t, tracker, 96);
    *owned = whisk::IsOwnWhiskTracker(t, Scalar::FromMont(k)) ? 1 : 0;
    return CURDLE_OK;
  });
}

extern "C" int curdle_whisk_compute_tracker(const uint64_t k[4], const uint64_t r[4], uint8_t* tracker_out) {
  if (!k || !r || !tracker_out) return curdle_set_last_error(CURDLE_EINVAL, "null argument");
  return Guard([&]() {
    const whisk::WhiskTracker t = whisk::ComputeWhiskTracker(Scalar::FromMont(k), Scalar::FromMont(r));
    memcpy(tracker_out, &t, 96);
    return CURDLE_OK;
  });
}

extern "C" int curdle_whisk_k_commitment(const uint64_t k[4], uint8_t* out) {
  if (!k || !out) return curdle_set_last_error(CURDLE_EINVAL, "null argument");
  return Guard([&]() {
    whisk::WhiskKCommitment(Scalar::FromMont(k), out);
    return CURDLE_OK;
  });
}

extern "C" int curdle_verify_set_eager(int eager) { return proto::SetEagerChecks(eager); }

// Round trip of the wire format: decode, re-encode (curdleproof_test.go "encode/decode").
extern "C" int curdle_proof_reencode(const uint8_t* proof, size_t proof_len, uint8_t* out, size_t cap, size_t* out_len) {
  if (!proof || !out_len) return curdle_set_last_error(CURDLE_EINVAL, "null argument");
  return Guard([&]() {
    proto::Proof p = proto::Proof::FromBytes(proof, proof_len, /*subgroup_check=*/true);
    std::vector<uint8_t> bytes = p.Serialize();
    *out_len = bytes.size();
    if (!out || cap < bytes.size()) return curdle_set_last_error(CURDLE_EINVAL, "buffer too small");
    memcpy(out, bytes.data(), bytes.size());
    return CURDLE_OK;
  });
}

// common.IPA (/root/reference/common/util.go:26-35): inner product of two Fr vectors, Montgomery
// limbs in and out; the reference's own known answer (common/util_test.go:10-27) is asserted
// against this entry point.
extern "C" int curdle_fr_inner_product(const uint64_t* a, size_t a_len, const uint64_t* b, size_t b_len,
                                       uint64_t out_fr[4]) {
  if (!out_fr || (a_len && !a) || (b_len && !b)) return curdle_set_last_error(CURDLE_EINVAL, "null argument");
  return Guard([&]() {
    std::vector<Scalar> va(a_len), vb(b_len);
    for (size_t i = 0; i < a_len; i++) va[i] = Scalar::FromMont(a + 4 * i);
    for (size_t i = 0; i < b_len; i++) vb[i] = Scalar::FromMont(b + 4 * i);
    const Scalar r = alg::InnerProduct(va, vb);  // throws on a length mismatch, as util.go:27-29 errors
    memcpy(out_fr, &r.v, 32);
    return CURDLE_OK;
  });
}

// transcript pieces exposed for the known-answer test of the Merlin construction
extern "C" int curdle_merlin_test_vector(const char* protocol, const char* label, const uint8_t* msg, size_t msg_len,
                                         const char* challenge_label, uint8_t* out, size_t out_len) {
  if (!protocol || !label || !challenge_label || !out) return curdle_set_last_error(CURDLE_EINVAL, "null argument");
  transcript::Merlin m(protocol);
  m.AppendMessage(label, msg, msg_len);
  m.ChallengeBytes(challenge_label, out, out_len);
  return CURDLE_OK;
}

// G1 compressed encoding helpers (gnark G1Affine.Bytes / SetBytes)
extern "C" int curdle_g1_compress(const uint64_t jac[18], uint8_t out[48]) {
  if (!jac || !out) return curdle_set_last_error(CURDLE_EINVAL, "null argument");
  Point::FromJac(jac).Compressed(out);
  return CURDLE_OK;
}
extern "C" int curdle_g1_decompress(const uint8_t in[48], int subgroup_check, uint64_t out_jac[18]) {
  if (!in || !out_jac) return curdle_set_last_error(CURDLE_EINVAL, "null argument");
  Point p;
  if (!Point::FromCompressed(in, &p, subgroup_check != 0)) return curdle_set_last_error(CURDLE_EINVAL, "invalid point");
  p.Jac(out_jac);
  return CURDLE_OK;
}
