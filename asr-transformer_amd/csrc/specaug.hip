// SpecAugment on the device (asrx_specaug): a time warp plus frequency and time masks, applied while the spectrogram
// is copied (B, 1, F, T) fp32 -> (B, 1, F, T) fp32, one launch.  The rule is DESIGN.md §16, restated in numpy by
// tests/specaug_ref.py: every random decision of utterance b is a draw rng_hash(s, b * D + j) with s the seed of the
// step (seed_at), so step n's augmentation is a pure function of (seed, n, b).
//
// Each workgroup derives its utterance's plan itself (at most 34 hashes by its first wave, into LDS, then a barrier):
// no table launch in front, no round trip.  A workgroup covers SA_RUN frames of SA_ROWS frequency rows.  Masked
// elements are stored without reading the source.  Without a warp and with 16-B aligned rows the copy moves 16 B
// per lane; otherwise (and with a warp: two gathered reads per output, the source index monotone in t) 4 B per lane,
// consecutive lanes on consecutive frames.
#include "common.h"

constexpr int SA_RUN = ASRX_SPECAUG_RUN;          // frames per workgroup
constexpr int SA_ROWS = 4;                        // frequency rows per workgroup
constexpr int SA_MAXM = ASRX_SPECAUG_MAX_MASKS;   // masks of each kind
static_assert(SA_RUN == 256 * 4, "one 16-B access per lane and row");

struct SaArgs {
  const float* src;
  float* dst;
  const int32_t* lengths;
  int32_t* plan_out;
  int64_t sb, db;
  uint64_t seed, step;
  int F, T, nF, Wf, nT, Wt, W;
  float ratio, mask_value;
};

struct SaPlan {
  int L, w0, c;   // c == 0: no warp
  int f0[SA_MAXM], fw[SA_MAXM], t0[SA_MAXM], tw[SA_MAXM];
};

// integer uniform on [0, n): (uint64(h) * n) >> 32
ASRX_DEV int sa_uniform(uint32_t h, int n) { return (int)__umulhi(h, (uint32_t)n); }

// The plan of utterance b into P (LDS), by the first wave; every thread of the workgroup calls this (barrier inside).
ASRX_DEV void sa_plan(const SaArgs& a, int b, uint32_t* sh, SaPlan& P) {
  const int tid = threadIdx.x;
  if (tid < 64) {
    const int D = 2 + 2 * (a.nF + a.nT);
    const uint64_t s = seed_at(a.seed, a.step);
    if (tid < D) sh[tid] = rng_hash(s, (uint32_t)(b * D + tid));
    wave_lds_sync();
    const int L = a.lengths ? clamp_len(a.lengths[b], a.T) : a.T;
    if (tid == 0) {
      int w0 = 0, c = 0;
      if (a.W > 0 && L - a.W > a.W) {
        w0 = a.W + sa_uniform(sh[0], L - 2 * a.W);
        c = w0 - a.W + 1 + sa_uniform(sh[1], 2 * a.W);   // 1 <= c <= L - 1
      }
      P.L = L;
      P.w0 = w0;
      P.c = c;
    } else if (tid <= a.nF) {
      const int j = tid - 1;
      const int w = sa_uniform(sh[2 + 2 * j], min(a.Wf, a.F) + 1);
      P.fw[j] = w;
      P.f0[j] = sa_uniform(sh[3 + 2 * j], a.F - w + 1);
    } else if (tid <= a.nF + a.nT) {
      const int j = tid - 1 - a.nF;
      const int cap = min(a.Wt, (int)floorf(a.ratio * (float)L));
      const int w = sa_uniform(sh[2 + 2 * a.nF + 2 * j], cap + 1);
      P.tw[j] = w;
      P.t0[j] = sa_uniform(sh[3 + 2 * a.nF + 2 * j], L - w + 1);
    }
  }
  __syncthreads();
  if (a.plan_out && blockIdx.x == 0 && blockIdx.y == 0) {   // one workgroup per utterance writes the row
    const int n = 4 + 2 * (a.nF + a.nT);
    if (tid < n) {
      int v;
      if (tid < 4) {
        v = tid == 0 ? P.L : (tid == 1 ? P.w0 : (tid == 2 ? P.c : 0));
      } else {
        const int m = (tid - 4) >> 1, second = (tid - 4) & 1;
        if (m < a.nF) v = second ? P.fw[m] : P.f0[m];
        else v = second ? P.tw[m - a.nF] : P.t0[m - a.nF];
      }
      a.plan_out[(int64_t)b * n + tid] = v;
    }
  }
}

// VEC: no utterance is warped, every row of src and dst starts 16-B aligned and T % 4 == 0
template <bool VEC>
__global__ __launch_bounds__(256) void specaug_kernel(SaArgs a) {
  __shared__ uint32_t sh[64];
  __shared__ SaPlan P;
  const int b = blockIdx.z, tid = threadIdx.x;
  sa_plan(a, b, sh, P);
  const int L = P.L, T = a.T;
  const int fbase = blockIdx.y * SA_ROWS;
  const int nrows = min(SA_ROWS, a.F - fbase);
  unsigned rowm = 0;   // bit r: row fbase + r lies in a frequency mask
  for (int j = 0; j < a.nF; ++j) {
    const int f0 = P.f0[j], f1 = f0 + P.fw[j];
#pragma unroll
    for (int r = 0; r < SA_ROWS; ++r)
      if (fbase + r >= f0 && fbase + r < f1) rowm |= 1u << r;
  }
  const float* sp = a.src + (int64_t)b * a.sb + (int64_t)fbase * T;
  float* dp = a.dst + (int64_t)b * a.db + (int64_t)fbase * T;
  const float mv = a.mask_value;

  if constexpr (VEC) {
    const int t = blockIdx.x * SA_RUN + tid * 4;
    if (t >= T) return;
    unsigned tm = 0, live = 0;   // bit k: frame t + k lies in a time mask / in front of L
    for (int j = 0; j < a.nT; ++j) {
      const int t0 = P.t0[j], t1 = t0 + P.tw[j];
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (t + k >= t0 && t + k < t1) tm |= 1u << k;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (t + k < L) live |= 1u << k;
    f4_t v[SA_ROWS] = {};
    unsigned m[SA_ROWS];
#pragma unroll
    for (int r = 0; r < SA_ROWS; ++r) {
      m[r] = ((rowm >> r & 1u) ? 0xFu : tm) & live;
      if (r < nrows && m[r] != 0xFu) v[r] = *(const f4_t*)(sp + (int64_t)r * T + t);
    }
#pragma unroll
    for (int r = 0; r < SA_ROWS; ++r) {
      if (r >= nrows) break;
      f4_t o;
#pragma unroll
      for (int k = 0; k < 4; ++k) o[k] = (m[r] >> k & 1u) ? mv : v[r][k];
      *(f4_t*)(dp + (int64_t)r * T + t) = o;
    }
  } else {
    const int c = P.c, w0 = P.w0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int t = blockIdx.x * SA_RUN + k * 256 + tid;
      if (t >= T) break;
      bool tmask = false;
      for (int j = 0; j < a.nT; ++j) tmask |= t >= P.t0[j] && t < P.t0[j] + P.tw[j];
      const bool live = t < L;
      if (c == 0 || !live) {   // plain copy under the masks; the padding bit for bit
#pragma unroll
        for (int r = 0; r < SA_ROWS; ++r) {
          if (r >= nrows) break;
          const bool masked = live && (tmask || (rowm >> r & 1u));
          dp[(int64_t)r * T + t] = masked ? mv : sp[(int64_t)r * T + t];
        }
        continue;
      }
      // source position of output frame t: i + frac, piecewise linear through (0, 0), (c, w0), (L, L)
      const int lo = t < c ? 0 : c, base = t < c ? 0 : w0;
      const int mul = t < c ? w0 : L - w0, den = t < c ? c : L - c;
      int i, r_;
      if (L <= 65535) {   // num < L * L fits 32 bits: the quotient and remainder of the 64-bit rule
        const uint32_t num = (uint32_t)(t - lo) * (uint32_t)mul;
        i = base + (int)(num / (uint32_t)den);
        r_ = (int)(num % (uint32_t)den);
      } else {
        const uint64_t num = (uint64_t)(t - lo) * (uint64_t)mul;
        i = base + (int)(num / (uint64_t)den);
        r_ = (int)(num % (uint64_t)den);
      }
      const float frac = (float)r_ / (float)den;
      const int i1 = min(i + 1, L - 1);
#pragma unroll
      for (int r = 0; r < SA_ROWS; ++r) {
        if (r >= nrows) break;
        float o = mv;
        if (!(tmask || (rowm >> r & 1u))) {
          const float x0 = sp[(int64_t)r * T + i], x1 = sp[(int64_t)r * T + i1];
          o = x0 + frac * (x1 - x0);
        }
        dp[(int64_t)r * T + t] = o;
      }
    }
  }
}

extern "C" int asrx_specaug(const float* src, float* dst, int32_t B, int32_t F, int32_t T, int64_t src_bstride,
                            int64_t dst_bstride, const int32_t* lengths, int32_t freq_masks, int32_t freq_width,
                            int32_t time_masks, int32_t time_width, float time_ratio, int32_t time_warp,
                            float mask_value, uint64_t seed, uint64_t step, int32_t* plan_out, void* stream) {
  if (!src || !dst || (const float*)dst == src) return ASRX_ERR_ARG;
  if ((((uintptr_t)src | (uintptr_t)dst) & 3) != 0) return ASRX_ERR_ARG;
  if (F < 1 || T < 1 || B < 0) return ASRX_ERR_ARG;
  if (freq_masks < 0 || freq_width < 0 || time_masks < 0 || time_width < 0 || time_warp < 0) return ASRX_ERR_ARG;
  if (!(time_ratio >= 0.f && time_ratio <= 1.f)) return ASRX_ERR_ARG;
  if (freq_masks > SA_MAXM || time_masks > SA_MAXM || B > 65535) return ASRX_ERR_UNSUPPORTED;
  if (F > 65535 * SA_ROWS) return ASRX_ERR_UNSUPPORTED;
  if (B == 0) return ASRX_OK;
  const int64_t plane = (int64_t)F * T;
  if (B > 1 && (src_bstride < plane || dst_bstride < plane)) return ASRX_ERR_ARG;
  // the warp reads neighbouring frames: the two extents must not overlap
  const uintptr_t s0 = (uintptr_t)src, d0 = (uintptr_t)dst;
  const uintptr_t s1 = s0 + (uintptr_t)((int64_t)(B - 1) * src_bstride + plane) * sizeof(float);
  const uintptr_t d1 = d0 + (uintptr_t)((int64_t)(B - 1) * dst_bstride + plane) * sizeof(float);
  if (s0 < d1 && d0 < s1) return ASRX_ERR_ARG;
  SaArgs a;
  a.src = src; a.dst = dst; a.lengths = lengths; a.plan_out = plan_out;
  a.sb = src_bstride; a.db = dst_bstride; a.seed = seed; a.step = step;
  a.F = F; a.T = T; a.nF = freq_masks; a.Wf = freq_width; a.nT = time_masks; a.Wt = time_width; a.W = time_warp;
  a.ratio = time_ratio; a.mask_value = mask_value;
  const bool vec = time_warp == 0 && ((s0 | d0) & 15) == 0 && T % 4 == 0 &&
                   (B == 1 || (src_bstride % 4 == 0 && dst_bstride % 4 == 0));
  const dim3 grid(cdiv(T, SA_RUN), cdiv(F, SA_ROWS), (unsigned)B);
  if (vec) hipLaunchKernelGGL(specaug_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, a);
  else hipLaunchKernelGGL(specaug_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, a);
  ASRX_CHECK_LAUNCH();
  return ASRX_OK;
}
