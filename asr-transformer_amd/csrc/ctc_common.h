// What the CTC, beam and scoring kernels share beyond common.h's wave primitives: the log2-domain helpers and the
// host-side (blank, label) pair plumbing of the two chain kernels (ctc.hip, ctc_align.hip).
#pragma once
#include "common.h"

#include <type_traits>

constexpr float kLog2e = 1.4426950408889634f;
constexpr float kLn2 = 0.6931471805599453f;

// raw v_log_f32 (log2 x)
ASRX_DEV float log2_raw(float x) { return __builtin_amdgcn_logf(x); }

// log2(2^a + 2^b) and log2(2^a + 2^b + 2^c); -inf operands (and all -inf) are legal
ASRX_DEV float lae2(float a, float b) {
  const float hi = fmaxf(a, b), lo = fminf(a, b);
  const float hs = hi == -INFINITY ? 0.f : hi;
  return hi + log2_raw(1.f + exp2_raw(lo - hs));
}
ASRX_DEV float lae3(float a, float b, float c) {
  const float hi = fmaxf(fmaxf(a, b), c), lo = fminf(fminf(a, b), c);
  const float mid = __builtin_amdgcn_fmed3f(a, b, c);
  const float hs = hi == -INFINITY ? 0.f : hi;
  return hi + log2_raw(1.f + exp2_raw(mid - hs) + exp2_raw(lo - hs));
}

// ---- (blank, label) pairs: a sample's 2L + 1 extended states are L + 1 pairs, lane i of one wave owning the pairs
// i*KP .. i*KP + KP - 1 in registers, KP = ceil((Lmax + 1) / 64) <= 4.  The per-lane pair setup and the four-frame
// emission prefetch of ctc_chain_kernel and ctc_align_kernel are deliberately NOT shared: one reads validated targets,
// has a direction and carries (max, log2 sum), the other validates in place and carries one logsumexp, and a template
// over all of that would be more machinery than the two loops.
constexpr int CTC_MAXL = 255;   // L + 1 <= 256 pairs = 64 lanes x 4

inline int ctc_kp(int max_l) { return max_l / 64 + 1; }   // = ceil((max_l + 1) / 64) for max_l >= 0, no overflow

// f(std::integral_constant<int, KP>) for the kernel instance of kp = 1 .. 4
template <typename F> void ctc_dispatch_kp(int kp, F&& f) {
  switch (kp) {
    case 1: f(std::integral_constant<int, 1>()); break;
    case 2: f(std::integral_constant<int, 2>()); break;
    case 3: f(std::integral_constant<int, 3>()); break;
    default: f(std::integral_constant<int, 4>()); break;
  }
}

// The argument checks asrx_ctc_loss and asrx_ctc_align share, in the order both keep; own_ok: the entry point's own
// pointer and workspace checks, which stand between the targets' pointer rule and the size limits.
inline int ctc_check_target_args(int32_t B, int32_t T, int32_t V, int64_t ld, const int64_t* targets,
                                 int64_t tgt_stride, int32_t max_target_len, int32_t blank, bool own_ok) {
  if (B <= 0 || T <= 0 || V <= 0 || ld < V || max_target_len < 0 || tgt_stride < 0) return ASRX_ERR_ARG;
  if (blank < 0 || blank >= V) return ASRX_ERR_ARG;
  if (max_target_len > CTC_MAXL) return ASRX_ERR_UNSUPPORTED;
  if (tgt_stride < max_target_len) return ASRX_ERR_ARG;
  if (!own_ok || (max_target_len > 0 && !targets)) return ASRX_ERR_ARG;
  if ((int64_t)B * T > 0x7fffffffLL / 4 || B > 65535) return ASRX_ERR_UNSUPPORTED;
  return ASRX_OK;
}

// targets may be null with max_target_len = 0: the kernels still take a pointer (never read, every length is 0)
inline const int64_t* ctc_targets_or_dummy(const int64_t* targets) {
  static const int64_t no_targets[1] = {0};
  return targets ? targets : no_targets;
}
