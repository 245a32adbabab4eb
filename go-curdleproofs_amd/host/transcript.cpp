// Merlin / STROBE-128 transcript and the reference's wrapper -- see transcript.h.
#include "transcript.h"

#include "keccak.h"
#include "knobs.h"
#include "transcript_batch.h"

#include <string.h>

#include <atomic>
#include <thread>

namespace curdle {
namespace transcript {

// Keccak-f[1600] on STROBE's byte state (little-endian lanes; keccak.h has the round; the
// state is 8-byte aligned in the class).
static void keccak_f1600(uint8_t st8[200]) { curdle::keccak_f1600_dispatch(reinterpret_cast<uint64_t*>(st8)); }

// ---------------------------------------------------------------- STROBE ---
static constexpr uint8_t kStrobeR = 166;
static constexpr uint8_t FLAG_I = 1, FLAG_A = 1 << 1, FLAG_C = 1 << 2, FLAG_M = 1 << 4, FLAG_K = 1 << 5;

Strobe128::Strobe128(const std::string& protocol_label) : pos_(0), pos_begin_(0), cur_flags_(0) {
  memset(st_, 0, sizeof(st_));
  const uint8_t init[6] = {1, (uint8_t)(kStrobeR + 2), 1, 0, 1, 96};
  memcpy(st_, init, 6);
  memcpy(st_ + 6, "STROBEv1.0.2", 12);
  keccak_f1600(st_);
  MetaAd(reinterpret_cast<const uint8_t*>(protocol_label.data()), protocol_label.size(), false);
}

Strobe128::Strobe128(Exported e) : pos_(e.bytes[200]), pos_begin_(e.bytes[201]), cur_flags_(e.bytes[202]) {
  memcpy(st_, e.bytes, 200);
}

void Strobe128::Export(uint8_t out[208]) const {
  memcpy(out, st_, 200);
  out[200] = pos_;
  out[201] = pos_begin_;
  out[202] = cur_flags_;
  memset(out + 203, 0, 5);
}

void Strobe128::RunF() {
  st_[pos_] ^= pos_begin_;
  st_[pos_ + 1] ^= 0x04;
  st_[kStrobeR + 1] ^= 0x80;
  keccak_f1600(st_);
  pos_ = 0;
  pos_begin_ = 0;
}

// One verification absorbs ~115 KB in ~1,500 messages: whole runs up to the rate boundary at a
// time, not byte by byte.
void Strobe128::Absorb(const uint8_t* data, size_t len) {
  while (len) {
    size_t run = (size_t)(kStrobeR - pos_);
    if (run > len) run = len;
    for (size_t i = 0; i < run; i++) st_[pos_ + i] ^= data[i];  // vectorised by the compiler
    pos_ = (uint8_t)(pos_ + run);
    data += run;
    len -= run;
    if (pos_ == kStrobeR) RunF();
  }
}

void Strobe128::Squeeze(uint8_t* out, size_t len) {
  while (len) {
    size_t run = (size_t)(kStrobeR - pos_);
    if (run > len) run = len;
    memcpy(out, st_ + pos_, run);
    memset(st_ + pos_, 0, run);
    pos_ = (uint8_t)(pos_ + run);
    out += run;
    len -= run;
    if (pos_ == kStrobeR) RunF();
  }
}

void Strobe128::BeginOp(uint8_t flags, bool more) {
  if (more) return;  // continuation of the current operation (same flags)
  const uint8_t old_begin = pos_begin_;
  pos_begin_ = pos_ + 1;
  cur_flags_ = flags;
  const uint8_t hdr[2] = {old_begin, flags};
  Absorb(hdr, 2);
  const bool force_f = (flags & (FLAG_C | FLAG_K)) != 0;
  if (force_f && pos_ != 0) RunF();
}

void Strobe128::MetaAd(const uint8_t* data, size_t len, bool more) {
  BeginOp(FLAG_M | FLAG_A, more);
  Absorb(data, len);
}
void Strobe128::Ad(const uint8_t* data, size_t len, bool more) {
  BeginOp(FLAG_A, more);
  Absorb(data, len);
}
void Strobe128::Prf(uint8_t* out, size_t len, bool more) {
  BeginOp(FLAG_I | FLAG_A | FLAG_C, more);
  Squeeze(out, len);
}

// ---------------------------------------------------------------- Merlin ---
static void le32(uint8_t out[4], size_t v) {
  out[0] = (uint8_t)v;
  out[1] = (uint8_t)(v >> 8);
  out[2] = (uint8_t)(v >> 16);
  out[3] = (uint8_t)(v >> 24);
}

Merlin::Merlin(const std::string& label) : strobe_("Merlin v1.0") {
  AppendMessage("dom-sep", reinterpret_cast<const uint8_t*>(label.data()), label.size());
}

void Merlin::AppendMessage(const std::string& label, const uint8_t* msg, size_t len) {
  uint8_t n[4];
  le32(n, len);
  strobe_.MetaAd(reinterpret_cast<const uint8_t*>(label.data()), label.size(), false);
  strobe_.MetaAd(n, 4, true);
  strobe_.Ad(msg, len, false);
}

void Merlin::ChallengeBytes(const std::string& label, uint8_t* out, size_t len) {
  uint8_t n[4];
  le32(n, len);
  strobe_.MetaAd(reinterpret_cast<const uint8_t*>(label.data()), label.size(), false);
  strobe_.MetaAd(n, 4, true);
  strobe_.Prf(out, len, false);
}

// ------------------------------------------------------------- Transcript ---
void Transcript::AppendPoint(const std::string& label, const alg::Point& p) {
  uint8_t b[48];
  p.Compressed(b);
  inner_.AppendMessage(label, b, 48);  // transcript.go:34-38
}
void Transcript::AppendPoints(const std::string& label, const std::vector<alg::Point>& points) {
  for (const auto& p : points) AppendPoint(label, p);  // :25-30 (normalise, then one message per point)
}
void Transcript::AppendPointsAffine(const std::string& label, const std::vector<G1Affine>& points) {
  std::vector<uint8_t> b(48 * points.size());
  alg::CompressAffineBatch(points.data(), points.size(), b.data());
  AppendCompressed(label, b.data(), points.size());
}
void Transcript::AppendCompressed(const std::string& label, const uint8_t* records, size_t count) {
  for (size_t i = 0; i < count; i++) inner_.AppendMessage(label, records + 48 * i, 48);
}
void Transcript::AppendScalar(const std::string& label, const alg::Scalar& s) {
  uint8_t b[32];
  s.Bytes(b);
  inner_.AppendMessage(label, b, 32);  // :41-46
}
void Transcript::AppendScalars(const std::string& label, const std::vector<alg::Scalar>& scalars) {
  for (const auto& s : scalars) AppendScalar(label, s);
}
alg::Scalar Transcript::GetAndAppendChallenge(const std::string& label) {
  for (;;) {  // :48-58: 32 bytes, canonical or retry, then re-append under the same label
    uint8_t dest[32];
    inner_.ChallengeBytes(label, dest, 32);
    alg::Scalar c;
    if (alg::Scalar::SetBytesCanonical(dest, &c)) {
      AppendScalar(label, c);
      return c;
    }
  }
}
std::vector<alg::Scalar> Transcript::GetAndAppendChallenges(const std::string& label, size_t count) {
  std::vector<alg::Scalar> out;
  out.reserve(count);
  for (size_t i = 0; i < count; i++) out.push_back(GetAndAppendChallenge(label));
  return out;
}

}  // namespace transcript
}  // namespace curdle

// ------------------------------------------------- batched transcripts ---
// transcript_batch.h: the checks of a call, the tape of a program, the host twin.
namespace curdle {
namespace transcript {
namespace {
// Strobe128 over positions instead of a state: what it would xor where, block by block.
struct SymStrobe {
  uint8_t pos, pos_begin, cur_flags;
  uint8_t cbytes[8 * kRateWords];
  long long src[8 * kRateWords];  // member byte that enters at this state byte, or -1
  std::vector<TapeBlock>* pool;
  size_t perms = 0;
  bool ok = true;  // false: two runs of member bytes in one rate word (framing is >= 8 bytes: cannot happen)

  SymStrobe(const uint8_t start[3], std::vector<TapeBlock>* p) : pos(start[0]), pos_begin(start[1]), cur_flags(start[2]), pool(p) { Clear(); }
  void Clear() {
    memset(cbytes, 0, sizeof(cbytes));
    for (long long& v : src) v = -1;
  }
  bool Dirty() const {
    for (size_t i = 0; i < sizeof(cbytes); i++)
      if (cbytes[i] || src[i] >= 0) return true;
    return false;
  }
  void Emit(bool run_f) {
    TapeBlock b;
    memset(&b, 0, sizeof(b));
    b.run_f = run_f ? 1 : 0;
    for (int w = 0; w < kRateWords; w++) {
      long long delta = -1;
      for (int j = 0; j < 8; j++) {
        b.w[w].cmask |= (uint64_t)cbytes[8 * w + j] << (8 * j);
        const long long sv = src[8 * w + j];
        if (sv < 0) continue;
        b.w[w].dmask |= (uint64_t)0xff << (8 * j);
        const long long t = sv - j + 8;  // the row starts with 8 zero bytes: t >= 1
        if (delta >= 0 && t != delta) ok = false;
        delta = t;
      }
      if (delta >= 0) {
        b.w[w].idx = (uint32_t)(delta >> 3);
        b.w[w].sh = (uint32_t)(delta & 7) * 8;
      }
    }
    pool->push_back(b);
    Clear();
  }
  void RunF() {
    cbytes[pos] ^= pos_begin;
    cbytes[pos + 1] ^= 0x04;
    cbytes[kStrobeR + 1] ^= 0x80;
    Emit(true);
    perms++;
    pos = 0;
    pos_begin = 0;
  }
  void AbsorbConst(const uint8_t* d, size_t len) {
    for (size_t i = 0; i < len; i++) {
      cbytes[pos++] ^= d[i];
      if (pos == kStrobeR) RunF();
    }
  }
  void AbsorbData(size_t off, size_t len) {
    for (size_t i = 0; i < len; i++) {
      src[pos++] = (long long)(off + i);
      if (pos == kStrobeR) RunF();
    }
  }
  void BeginOp(uint8_t flags) {
    const uint8_t hdr[2] = {pos_begin, flags};
    pos_begin = pos + 1;
    cur_flags = flags;
    AbsorbConst(hdr, 2);
    if ((flags & (FLAG_C | FLAG_K)) != 0 && pos != 0) RunF();
  }
  // Merlin's framing of a message or a challenge of `len` bytes under `label`, up to and including the header of
  // the operation `flags` that carries the bytes themselves
  void Frame(const char* label, size_t label_len, size_t len, uint8_t flags) {
    uint8_t n[4];
    le32(n, len);
    BeginOp(FLAG_M | FLAG_A);
    AbsorbConst(reinterpret_cast<const uint8_t*>(label), label_len);
    AbsorbConst(n, 4);
    BeginOp(flags);
  }
};
constexpr uint8_t kFlagsAd = FLAG_A, kFlagsPrf = FLAG_I | FLAG_A | FLAG_C;
}  // namespace

int CheckBatchCall(const char* transcript_label, const uint8_t* init_states, const curdle_transcript_step* steps,
                   size_t n_steps, const uint8_t* data, size_t data_stride, size_t k, const uint8_t* challenges,
                   const uint8_t* status, uint8_t start[3], std::string* why) {
  auto bad = [&](const std::string& m) {
    *why = m;
    return CURDLE_EINVAL;
  };
  if ((transcript_label != nullptr) == (init_states != nullptr)) return bad("exactly one of transcript_label and init_states is given");
  if (n_steps && !steps) return bad("null argument");
  if (n_steps > CURDLE_TRANSCRIPT_MAX_MESSAGES) return bad("more steps than CURDLE_TRANSCRIPT_MAX_MESSAGES");
  if (k > CURDLE_TRANSCRIPT_MAX_MEMBERS) return bad("k = " + std::to_string(k) + " exceeds CURDLE_TRANSCRIPT_MAX_MEMBERS");
  size_t consumed = 0, messages = 0, n_ch = 0;
  for (size_t s = 0; s < n_steps; s++) {
    const curdle_transcript_step& st = steps[s];
    if (st.op != CURDLE_TR_APPEND && st.op != CURDLE_TR_CHALLENGES) return bad("step " + std::to_string(s) + ": unknown op " + std::to_string(st.op));
    if (st.label_len > 32) return bad("step " + std::to_string(s) + ": label_len above 32");
    messages += st.count;
    if (messages > CURDLE_TRANSCRIPT_MAX_MESSAGES) return bad("more messages and challenges than CURDLE_TRANSCRIPT_MAX_MESSAGES");
    if (st.op == CURDLE_TR_APPEND) {
      if (st.len > CURDLE_TRANSCRIPT_MAX_BYTES) return bad("step " + std::to_string(s) + ": len above CURDLE_TRANSCRIPT_MAX_BYTES");
      consumed += (size_t)st.count * st.len;  // <= 2^16 * 2^20
      if (consumed > CURDLE_TRANSCRIPT_MAX_BYTES) return bad("the program reads more than CURDLE_TRANSCRIPT_MAX_BYTES per member");
    } else {
      n_ch += st.count;
      if (n_ch > CURDLE_TRANSCRIPT_MAX_CHALLENGES) return bad("more challenges than CURDLE_TRANSCRIPT_MAX_CHALLENGES");
    }
  }
  if (data_stride < consumed) return bad("data_stride = " + std::to_string(data_stride) + " is below the " + std::to_string(consumed) + " bytes the program reads");
  if (k && ((consumed && !data) || (n_ch && !challenges) || !status)) return bad("null argument");
  if (transcript_label) {
    uint8_t st[208];
    Transcript(std::string(transcript_label)).inner().Export(st);
    memcpy(start, st + 200, 3);
  } else {
    for (size_t i = 0; i < k; i++) {
      const uint8_t* t = init_states + i * CURDLE_TRANSCRIPT_STATE_SIZE + 200;
      if (t[0] >= kStrobeR || t[1] > kStrobeR || t[3] || t[4] || t[5] || t[6] || t[7]) return bad("init_states[" + std::to_string(i) + "] is not an exported state");
      if (memcmp(t, init_states + 200, 3) != 0) return bad("init_states[" + std::to_string(i) + "] is at another position than init_states[0]: one program serves all members");
    }
    memset(start, 0, 3);
    if (k) memcpy(start, init_states + 200, 3);
  }
  return CURDLE_OK;
}

void CompileTape(const curdle_transcript_step* steps, size_t n_steps, const uint8_t start[3], Tape* out) {
  Tape& T = *out;
  T = Tape();
  SymStrobe sym(start, &T.pool);
  size_t run_begin = 0;
  auto flush_run = [&]() {
    if (T.pool.size() > run_begin) T.ctl.push_back(TapeCtl{kBlocks, (uint32_t)run_begin, (uint32_t)(T.pool.size() - run_begin), 0, 0, 0, {0, 0}});
    run_begin = T.pool.size();
  };
  for (size_t s = 0; s < n_steps; s++) {
    const curdle_transcript_step& st = steps[s];
    if (st.op == CURDLE_TR_APPEND) {
      for (uint32_t c = 0; c < st.count; c++) {
        sym.Frame(st.label, st.label_len, st.len, kFlagsAd);
        sym.AbsorbData(T.consumed, st.len);
        T.consumed += st.len;
      }
      continue;
    }
    // every try after the first, and the re-append, start at (32, 0): compiled once per step
    uint32_t retry_at = 0, retry_n = 0, append_at = 0;
    uint8_t after[3] = {0, 0, 0};
    for (uint32_t c = 0; c < st.count; c++) {
      sym.Frame(st.label, st.label_len, 32, kFlagsPrf);  // ends in the PRF's forced F (or the one the header ran into)
      flush_run();
      if (c == 0) {
        const uint8_t squeezed[3] = {32, 0, kFlagsPrf};
        SymStrobe retry(squeezed, &T.pool);
        retry_at = (uint32_t)T.pool.size();
        retry.Frame(st.label, st.label_len, 32, kFlagsPrf);
        retry_n = (uint32_t)T.pool.size() - retry_at;
        SymStrobe app(squeezed, &T.pool);
        append_at = (uint32_t)T.pool.size();
        app.Frame(st.label, st.label_len, 32, kFlagsAd);  // 40 + label_len <= 72 bytes in: no F
        app.Emit(false);
        after[0] = app.pos + 32;
        after[1] = app.pos_begin;
        after[2] = kFlagsAd;
        run_begin = T.pool.size();
      }
      T.ctl.push_back(TapeCtl{kChallenge, retry_at, retry_n, append_at, (uint32_t)(after[0] - 32), (uint32_t)T.n_challenges, {0, 0}});
      T.n_challenges++;
      sym.pos = after[0];
      sym.pos_begin = after[1];
      sym.cur_flags = after[2];
    }
  }
  if (sym.Dirty()) sym.Emit(false);
  flush_run();
  T.pos = sym.pos;
  T.pos_begin = sym.pos_begin;
  T.cur_flags = sym.cur_flags;
  T.permutations = sym.perms;
}

}  // namespace transcript
}  // namespace curdle

extern "C" int curdle_set_last_error(int code, const char* msg);  // csrc/msm_context.hip

extern "C" int curdle_transcript_batch_host(const char* transcript_label, const uint8_t* init_states,
                                            const curdle_transcript_step* steps, size_t n_steps, const uint8_t* data,
                                            size_t data_stride, size_t k, uint8_t* challenges, uint8_t* states,
                                            uint8_t* status, int nthreads) {
  using namespace curdle;
  using namespace curdle::transcript;
  uint8_t start[3];
  std::string why;
  if (CheckBatchCall(transcript_label, init_states, steps, n_steps, data, data_stride, k, challenges, status, start, &why))
    return curdle_set_last_error(CURDLE_EINVAL, why.c_str());
  if (k == 0) return CURDLE_OK;
  try {
    size_t n_ch = 0;
    std::vector<std::string> labels(n_steps);
    for (size_t s = 0; s < n_steps; s++) {
      labels[s].assign(steps[s].label, steps[s].label_len);
      if (steps[s].op == CURDLE_TR_CHALLENGES) n_ch += steps[s].count;
    }
    static_assert(kMaxTries == CURDLE_TRANSCRIPT_MAX_TRIES, "the header's bound is the twin's and the kernels'");
    const int max_tries = knobs::transcript_max_tries();  // kMaxTries unless test hook TRANSCRIPT_MAX_TRIES lowered it
    const Transcript fresh = transcript_label ? Transcript(std::string(transcript_label)) : Transcript(Strobe128::Exported{init_states});
    auto member = [&](size_t i) {
      Transcript t = transcript_label ? fresh : Transcript(Strobe128::Exported{init_states + i * CURDLE_TRANSCRIPT_STATE_SIZE});
      const uint8_t* d = data + i * data_stride;
      uint8_t* out = challenges + i * n_ch * 32;
      status[i] = 0;
      for (size_t s = 0; s < n_steps && !status[i]; s++) {
        for (uint32_t c = 0; c < steps[s].count && !status[i]; c++) {
          if (steps[s].op == CURDLE_TR_APPEND) {
            t.inner().AppendMessage(labels[s], d, steps[s].len);
            d += steps[s].len;
            continue;
          }
          int tries = 0;
          for (;; tries++) {  // GetAndAppendChallenge with its wait bounded
            if (tries == max_tries) {
              status[i] = 1;
              break;
            }
            uint8_t dest[32];
            t.inner().ChallengeBytes(labels[s], dest, 32);
            alg::Scalar sc;
            if (!alg::Scalar::SetBytesCanonical(dest, &sc)) continue;
            t.AppendScalar(labels[s], sc);
            sc.Bytes(out);
            break;
          }
          out += 32;
        }
      }
      if (states) t.inner().Export(states + i * CURDLE_TRANSCRIPT_STATE_SIZE);
    };
    const size_t nt = std::max<size_t>(1, std::min<size_t>(nthreads < 1 ? 1 : (size_t)nthreads, k));
    std::atomic<size_t> next{0};
    auto work = [&]() {
      for (size_t i = next.fetch_add(1); i < k; i = next.fetch_add(1)) member(i);
    };
    std::vector<std::thread> pool;
    for (size_t t = 1; t < nt; t++) pool.emplace_back(work);
    work();
    for (std::thread& th : pool) th.join();
  } catch (const std::exception& e) {
    return curdle_set_last_error(CURDLE_ENOMEM, e.what());
  }
  return CURDLE_OK;
}

