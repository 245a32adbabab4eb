// What the batched entry-point families of the C ABI share on the host side (the *_api.hip units, msm_entry.hip; the
// definitions are in msm_context.hip): the scoped hold of an MSM slot (SlotHold), the list of ranges a call overwrites
// on its way out because they held a secret (WipeList), the per-context device copy behind a handle (ResidentCopy),
// and two one-liners.  No kernel translation unit includes this file.
#pragma once
#include "msm_internal.h"

namespace curdle_api {
inline bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

// the body of every curdle_stat_* reader: n counters into out[]
int read_stats(unsigned long long* out, const std::atomic<unsigned long long>* counters, int n);

// What the flagged tracker-proof generator (tracker_api.hip) borrows from two other families.  fbase_api.hip: the
// generator's fixed-base table on context cx (built on first use, a user reference that generator_table_release gives
// back) and the counters of a completed pass of k_fbase_mul_ct; g1_mul_ct_api.hip: those of a pass of k_g1_mul_ct.
int generator_table_acquire(Ctx& cx, void** d_table);
void generator_table_release();
void count_fbase_ct_pass(size_t n);
void count_g1_mul_ct_pass(size_t n);
// (What the two constant-time MSM families share has a header of its own, msm_ct_call.h.)

// A free slot, marked as acquire_slot marks it, or -1: never waits, brings no context up and leaves the error text alone.
int try_acquire_slot(Ctx& cx);

// The places a call (or one pass of it) writes a secret to.  A range is noted BEFORE the first secret byte goes there,
// so that a failure half-way still wipes it; memory the caller owns (the resident forms' arrays) is never noted.
struct WipeList {
  struct Range {
    void* p;
    size_t bytes;
  };
  static constexpr int kMax = 4;
  hipStream_t st;
  Range dev[kMax], host[kMax];
  int ndev = 0, nhost = 0;
  bool lost = false;  // a range did not fit: wipe() says so
  explicit WipeList(hipStream_t stream) : st(stream) {}
  void note_device(void* p, size_t bytes) { note(dev, ndev, p, bytes); }
  void note_host(void* p, size_t bytes) { note(host, nhost, p, bytes); }
  void note(Range* list, int& n, void* p, size_t bytes) {
    if (n < kMax)
      list[n++] = {p, bytes};
    else
      lost = true;
  }
  // Zeroes the device ranges on the stream, behind everything queued there, synchronises the stream in every case and
  // then zeroes the host ranges.  The first HIP error: CURDLE_EHIP, "<what>: <the error>".
  int wipe(const char* what);
};

// One MSM slot held for the length of a call: acquired by the constructor, given back by run().  A hold whose
// acquisition succeeded must be run.
class SlotHold {
 public:
  enum OnFailure { kSyncStreams, kDrainSlot };  // what a failed body is followed by: see run()
  SlotHold(Ctx& cx, bool block, void* user_stream) : cx_(cx), rc_(acquire_slot(cx, block, &a_)) {
    if (rc_ == CURDLE_OK) st_ = user_stream ? (hipStream_t)user_stream : slot().stream;
  }
  SlotHold(const SlotHold&) = delete;
  SlotHold& operator=(const SlotHold&) = delete;
  Slot& slot() { return cx_.slots[a_]; }
  hipStream_t stream() const { return st_; }  // the caller's stream if it gave one, the slot's otherwise
  // A second slot that only lends its stream and events, if one is free right now; null otherwise.
  Slot* try_second() {
    if (rc_ == CURDLE_OK && b_ < 0) b_ = try_acquire_slot(cx_);
    return b_ >= 0 ? &cx_.slots[b_] : nullptr;
  }
  void wipe_on_exit(WipeList* w, const char* what) { wipe_ = w, wipe_what_ = what; }
  // Sets the device and calls body().  After a failure nothing queued may outlive the hold: the held streams are
  // synchronised (or the slot drained).  Then the registered wipe, which synchronises too; then the slots go back,
  // the second one first.  A failed acquisition's status is returned as it is and the body does not run.
  template <class Body>
  int run(Body&& body, OnFailure on_failure = kSyncStreams) {
    if (rc_) return rc_;
    int rc = set_device();
    if (rc == CURDLE_OK) rc = body();
    return finish(rc, on_failure);
  }

 private:
  int set_device();
  int finish(int rc, OnFailure on_failure);
  Ctx& cx_;
  int a_ = -1, b_ = -1;
  int rc_;
  hipStream_t st_ = nullptr;
  WipeList* wipe_ = nullptr;
  const char* wipe_what_ = nullptr;
};

// The device copies of what a handle keeps in host memory (a resident base set, a fixed-base table): one per context,
// uploaded on first use there and again after a curdle_shutdown.  The handle owns one of these beside its host data;
// deleting the handle frees the copies.
struct ResidentCopy {
  struct Text {  // the family's wording of the three refusals
    const char* freed;      // the handle was freed while a call was in flight
    const char* shut_down;  // the context was shut down between the look and the upload
    const char* upload;     // "<upload>: <HIP error>"
  };
  // The family's part: allocate *dst on the context's device (selected already), fill it on `st` and synchronise
  // `st`.  Temporaries are the callable's own to free; *dst is freed by acquire() when the callable fails.
  using Upload = std::function<hipError_t(hipStream_t st, void** dst)>;
  std::mutex mu;
  void* d28[kMaxDevices] = {};       // per context
  unsigned epoch[kMaxDevices] = {};  // the context generation each copy belongs to
  int hipdev[kMaxDevices] = {};      // ... and the HIP device it was allocated on (a copy outlives its context: no device reset)
  int users = 0;                     // calls in flight that read a copy
  bool dead = false;                 // the free came while users > 0: the last user deletes
  // The copy on context cx (null where `upload` is empty and none was made); takes a user reference.
  int acquire(Ctx& cx, const Upload& upload, const Text& text, void** out);
  bool release();        // gives the reference back; true: the handle was freed meanwhile and the caller deletes it now
  bool free_or_defer();  // the owner's free: true: nobody reads a copy and the caller deletes the handle now
  ~ResidentCopy();
};
}  // namespace curdle_api
