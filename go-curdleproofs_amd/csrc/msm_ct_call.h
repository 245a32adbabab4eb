// What the two families of the constant-time MSM share on the host side: curdle_msm_g1_ct* (msm_ct_api.hip, which holds
// the definitions) and curdle_msm_g1_ct_bases* (msm_ct_bases_api.hip).  The limits, the refusals both state, the shape of
// a call of k segments, the staging of host scalars and the ONE body of a segmented call: this is the code that decides
// which ranges hold a secret and are wiped, and where the status word and the verdict live.  Host-only: no kernel
// translation unit includes this file.
#pragma once
#include "api_helpers.h"

namespace curdle_api {
constexpr size_t kMsmCtMaxTerms = 65536;  // terms of one call, and records of one base table: one pass, 256 blocks
constexpr size_t kMsmCtMaxBatch = 4096;   // MSMs of one call

int check_scalar_bits(unsigned bits);
// The verdict's refusal: the walks' status word came back set.
int refuse_scalar_range();
// curdle_stat_msm_ct_batch (calls, MSMs, level launches) by ONE completed batched call that ran the segmented sum.
void count_msm_ct_batch(size_t msms, unsigned levels);

// A call of k MSMs over pairs [offsets[0], offsets[k]) of the caller's arrays; a pair is `stride` terms: 1 for
// k_msm_ct_walk, Cb = ceil(scalar_bits / chunk_bits) for k_msm_ct_walk_rows.
struct SegShape {
  size_t k = 0, lo = 0, total = 0, nonempty = 0;  // MSMs | the first pair | pairs in all | MSMs with a pair
  unsigned stride = 1;
  std::vector<uint32_t> seg;     // (begin stride, count stride) per MSM, begin relative to the call's first pair: public
  std::vector<uint32_t> counts;  // count stride per MSM
  size_t terms() const { return total * stride; }
};
enum class TotalText { kPairs, kTerms };  // the family's wording of the total's refusal
// What a call refuses after its null arguments, in the order the public header states: scalar_bits, k, offsets that
// decrease, the total (total stride <= 65,536); the table is made behind that.  The single calls are offsets = {0, n}.
int seg_shape(const size_t* offsets, size_t k, unsigned bits, unsigned stride, TotalText text, SegShape* sh);

// The term workspace of a call, grown and noted on the WipeList: every form, before its walk.
int note_terms(Slot& S, WipeList& W, size_t terms);
// Host scalars on their way to the device: `copies` runs of the n records at `scalars` (32 bytes each) behind each other
// through the first pinned staging, which is grown to hold `behind` more bytes after them, into S.scalars.  Both ranges
// are on the WipeList before a byte of the scalars is written to either.
int stage_scalars(Slot& S, WipeList& W, const void* scalars, size_t n, size_t copies, size_t behind, hipStream_t st);

// The family's part of a segmented call, on the call's stream behind the zeroed status word and the table's upload: its
// own uploads of public data (h_extra: the pinned bytes it asked for) and its ONE walk launch, which writes sh.terms()
// terms into S.partials and ORs violations into *d_status.
using SegWalk = std::function<int(uint32_t* d_status, uint8_t* h_extra, hipStream_t st)>;
// One segmented call behind its checks and its staging, sh.total > 0.  The slot's small buffer holds the k results, the
// word the finish kernel copies the verdict to and -- from the next multiple of 16 -- the walk's status word; the second
// pinned staging holds the block that comes back (144 k + 4 bytes), from the status word's offset the (begin, count)
// table on its way into S.offsets, and from the next multiple of 16 the family's extra_bytes.  Then `walk`, the
// segmented sum, the ONE copy back, the wait and the verdict; out_jac is written on success only.  *levels: the level
// launches of the sum.  The counters are the caller's.
int seg_walk_sum_fetch(SlotHold& H, const SegShape& sh, size_t extra_bytes, uint64_t* out_jac, unsigned* levels, const SegWalk& walk);
}  // namespace curdle_api
