// Log-mel filterbank features and CMVN on the device (the rule is restated in numpy by
// tests/fbank_ref.py).
//
// asrx_logmel: waveform -> (log-)mel features [B][n_mels][frames], time innermost.  The STFT is asrx_spectrogram's
// fp32 MFMA GEMM into ws ([B][frames][2 nbins]); logmel_kernel replaces its square/transpose pass: it reads ws once,
// forms scale * (re^2 + im^2)^(power/2), applies the filterbank, the log, the global CMVN and the pad and stores the
// result transposed — the nbins-wide power spectrogram never reaches memory.  256 threads cover LM_FT = 32 frames of
// one utterance and every mel bin: chunks of LM_BC = 64 bins are loaded coalesced along bins (8 B per lane), turned
// through a padded LDS tile, and thread (f = tid & 31, g = tid >> 5) keeps the accumulators of filters m = g (mod 8)
// in registers across the chunks, walking only the part of the filter's bin range [lo, hi) that lies in the chunk, in
// ascending bin order.  The filters' nonzero column segments are packed into LDS once per workgroup (up to LM_WMAX
// weights, every triangular bank; a wider matrix is read from memory), so the inner loop reads LDS only, and the
// next chunk's loads are in flight while a chunk is filtered.  Stores have consecutive lanes on consecutive frames.
//
// asrx_cmvn: per-utterance (or given-statistics) normalisation of [B][F][T], one workgroup per (b, f) row; two passes
// (mean, then centred squares) over a row held in registers, reduced in a fixed tree.  asrx_feature_stats: fp64 sums
// for global CMVN, one workgroup per feature bin (an offline pass, not tuned).
#include <algorithm>
#include <cstring>

#include "common.h"

namespace {

constexpr int LM_FT = 32;                        // frames per workgroup
constexpr int LM_BC = 64;                        // bins per chunk
constexpr int LM_MAXM = ASRX_LOGMEL_MAX_MELS;    // filters
static_assert(LM_MAXM == 256, "one range per thread of the workgroup");

constexpr int LM_WMAX = 4096;                    // filter weights a workgroup packs into LDS (sum of hi - lo)

// the filters' bin ranges travel in the kernel arguments (validated on the host; 1.5 KiB); off[m] = sum of the widths
// of the filters in front of m: where filter m's weights lie in the packed LDS copy
struct LmRanges {
  uint16_t lo[LM_MAXM], hi[LM_MAXM], off[LM_MAXM];
};

struct LmArgs {
  const float* ws;
  const int32_t* wave_lengths;
  const float* fb;
  const float* mean;
  const float* istd;
  float* out;
  int32_t* frame_lengths;
  int64_t frames;
  int nbins, n_mels, n_fft, hop, power, log_mode;
  int wtotal;   // sum of the filters' widths if it fits LM_WMAX (the weights are packed into LDS), else 0
  float scale, log_mul, log_eps, pad_value;
};

// NJ: accumulators per thread, n_mels <= 8 NJ
template <int NJ>
__global__ __launch_bounds__(256) void logmel_kernel(LmArgs a, LmRanges r) {
  __shared__ float t[LM_BC][LM_FT + 1];
  __shared__ int s_lo[LM_MAXM], s_hi[LM_MAXM], s_off[LM_MAXM];
  __shared__ float wl[LM_WMAX];
  const int tid = threadIdx.x, b = blockIdx.y;
  const int64_t f0 = (int64_t)blockIdx.x * LM_FT;
  int64_t fr = a.frames;   // valid frames of this utterance
  if (a.wave_lengths) {
    const int len = a.wave_lengths[b];
    const int64_t v = len >= a.n_fft ? (int64_t)(len - a.n_fft) / a.hop + 1 : 0;
    fr = v < fr ? v : fr;
  }
  if (a.frame_lengths && blockIdx.x == 0 && tid == 0) a.frame_lengths[b] = (int32_t)fr;
  const int f = tid & 31, g = tid >> 5;
  const int64_t frames = a.frames;
  const int n_mels = a.n_mels, nbins = a.nbins;
  float* op = a.out + (int64_t)b * n_mels * frames + f0 + f;
  const bool inside = f0 + f < frames;
  if (f0 >= fr) {   // the whole tile is padding: nothing is loaded
    if (inside)
      for (int m = g; m < n_mels; m += 8) op[(int64_t)m * frames] = a.pad_value;
    return;
  }
  if (tid < n_mels) {
    s_lo[tid] = r.lo[tid];
    s_hi[tid] = r.hi[tid];
    s_off[tid] = r.off[tid];
  }
  const int wtotal = a.wtotal;
  if (wtotal > 0) {   // every filter's column segment fb[lo .. hi)[m], one after the other, into LDS
    __syncthreads();
    for (int idx = tid; idx < wtotal; idx += 256) {
      int m = 0, top = n_mels;   // the last filter with off[m] <= idx: off[m] <= idx < off[m] + width[m]
      while (top - m > 1) {
        const int mid = (m + top) >> 1;
        if (s_off[mid] <= idx) m = mid;
        else top = mid;
      }
      wl[idx] = a.fb[(int64_t)(s_lo[m] + idx - s_off[m]) * n_mels + m];
    }
  }
  float acc[NJ];
#pragma unroll
  for (int j = 0; j < NJ; ++j) acc[j] = 0.f;
  const float* cb = a.ws + (int64_t)b * frames * (2 * (int64_t)nbins);
  const int lb = tid & 63, lf = tid >> 6;   // load: bin n0 + lb, frames f0 + lf + 4 i
  float2 z[LM_FT / 4];   // the chunk in flight: loaded while the one before it is filtered
  auto load = [&](int n0) {
    const int n = n0 + lb;
#pragma unroll
    for (int i = 0; i < LM_FT / 4; ++i) {
      const int64_t fg = f0 + lf + 4 * i;
      z[i] = make_float2(0.f, 0.f);
      if (fg < fr && n < nbins) z[i] = *(const float2*)(cb + fg * (2 * (int64_t)nbins) + 2 * n);
    }
  };
  load(0);
  for (int n0 = 0; n0 < nbins; n0 += LM_BC) {
    __syncthreads();   // the previous chunk is consumed (first pass: the ranges and the weights are in LDS)
#pragma unroll
    for (int i = 0; i < LM_FT / 4; ++i) {   // (a frame or bin outside the data: zeros in, zero out)
      float v = z[i].x * z[i].x + z[i].y * z[i].y;
      if (a.power == 1) v = sqrtf(v);
      t[lb][lf + 4 * i] = v * a.scale;
    }
    __syncthreads();
    if (n0 + LM_BC < nbins) load(n0 + LM_BC);
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const int m = g + 8 * j;
      if (m < n_mels) {
        const int lo = max(s_lo[m], n0), hi = min(s_hi[m], n0 + LM_BC);
        float s = acc[j];
        if (wtotal > 0) {
          const int wb = s_off[m] - s_lo[m];
          for (int k = lo; k < hi; ++k) s = __builtin_fmaf(t[k - n0][f], wl[wb + k], s);
        } else {
          const float* w = a.fb + (int64_t)lo * n_mels + m;
          for (int k = lo; k < hi; ++k, w += n_mels) s = __builtin_fmaf(t[k - n0][f], *w, s);
        }
        acc[j] = s;
      }
    }
  }
  const bool pad = f0 + f >= fr;
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    const int m = g + 8 * j;
    if (m < n_mels && inside) {
      float v = acc[j];
      if (a.log_mode == 1) v = a.log_mul * logf(v + a.log_eps);
      else if (a.log_mode == 2) v = a.log_mul * logf(fmaxf(v, a.log_eps));
      if (a.mean) v -= a.mean[m];
      if (a.istd) v *= a.istd[m];
      op[(int64_t)m * frames] = pad ? a.pad_value : v;
    }
  }
}

// ---- CMVN

constexpr int CM_HOLD = 16;                  // elements a thread holds: rows of up to CM_ROW frames are read once
constexpr int CM_ROW = 256 * CM_HOLD;

struct CmArgs {
  const float* x;
  float* out;
  const int32_t* lengths;
  const float* mean;
  const float* istd;
  int64_t xb, ob;
  int T, norm_var;
  float eps, pad_value;
};

// the workgroup's sum in a fixed tree (wave ladder, then the four waves in LDS); every thread gets it
ASRX_DEV float cm_block_sum(float v, float* sh) {
  v = wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  return (sh[0] + sh[1]) + (sh[2] + sh[3]);
}

__global__ __launch_bounds__(256) void cmvn_kernel(CmArgs a) {
  __shared__ float sh[4];
  const int tid = threadIdx.x, fi = blockIdx.x, b = blockIdx.y, T = a.T;
  const int L = a.lengths ? clamp_len(a.lengths[b], T) : T;
  const float* xr = a.x + (int64_t)b * a.xb + (int64_t)fi * T;
  float* orow = a.out + (int64_t)b * a.ob + (int64_t)fi * T;
  const float pv = a.pad_value;
  if (a.mean || L == 0) {   // given statistics (global CMVN), or nothing to reduce
    const float mu = a.mean ? a.mean[fi] : 0.f, is = a.istd ? a.istd[fi] : 1.f;
    for (int t = tid; t < T; t += 256) orow[t] = t < L ? (xr[t] - mu) * is : pv;
    return;
  }
  const float rl = 1.f / (float)L;
  if (L <= CM_ROW) {
    float v[CM_HOLD];
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < CM_HOLD; ++k) {
      const int t = k * 256 + tid;
      v[k] = t < L ? xr[t] : 0.f;
      s += v[k];
    }
    const float mu = cm_block_sum(s, sh) * rl;   // (the barrier inside: every read of the row precedes every store)
    float q = 0.f;
#pragma unroll
    for (int k = 0; k < CM_HOLD; ++k) {
      const float d = k * 256 + tid < L ? v[k] - mu : 0.f;
      q = __builtin_fmaf(d, d, q);
    }
    const float var = cm_block_sum(q, sh) * rl;
    const float is = a.norm_var ? 1.f / fmaxf(sqrtf(var), a.eps) : 1.f;
#pragma unroll
    for (int k = 0; k < CM_HOLD; ++k) {
      const int t = k * 256 + tid;
      if (t < T) orow[t] = t < L ? (v[k] - mu) * is : pv;
    }
    for (int t = CM_ROW + tid; t < T; t += 256) orow[t] = pv;
    return;
  }
  // a row longer than the registers hold: three reads (the second and third come from the caches)
  float s = 0.f;
  for (int t = tid; t < L; t += 256) s += xr[t];
  const float mu = cm_block_sum(s, sh) * rl;
  float q = 0.f;
  for (int t = tid; t < L; t += 256) {
    const float d = xr[t] - mu;
    q = __builtin_fmaf(d, d, q);
  }
  const float var = cm_block_sum(q, sh) * rl;
  const float is = a.norm_var ? 1.f / fmaxf(sqrtf(var), a.eps) : 1.f;
  for (int t = tid; t < T; t += 256) orow[t] = t < L ? (xr[t] - mu) * is : pv;   // element t: this thread alone
}

// ---- running statistics for global CMVN: one workgroup per feature bin, fp64, fixed order

__global__ __launch_bounds__(256) void feature_stats_kernel(const float* __restrict__ x, int B, int T, int64_t xb,
                                                            const int32_t* __restrict__ lengths, double* sum,
                                                            double* sumsq, int64_t* count) {
  __shared__ double sh[8];
  const int tid = threadIdx.x, fi = blockIdx.x;
  double s = 0.0, q = 0.0;
  int64_t n = 0;
  for (int b = 0; b < B; ++b) {
    const int L = lengths ? clamp_len(lengths[b], T) : T;
    const float* xr = x + (int64_t)b * xb + (int64_t)fi * T;
    for (int t = tid; t < L; t += 256) {
      const double v = (double)xr[t];
      s += v;
      q += v * v;
    }
    n += L;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    s += __shfl_xor(s, o, 64);
    q += __shfl_xor(q, o, 64);
  }
  if ((tid & 63) == 0) {
    sh[tid >> 6] = s;
    sh[4 + (tid >> 6)] = q;
  }
  __syncthreads();
  if (tid == 0) {
    sum[fi] += (sh[0] + sh[1]) + (sh[2] + sh[3]);
    sumsq[fi] += (sh[4] + sh[5]) + (sh[6] + sh[7]);
    if (fi == 0) count[0] += n;
  }
}

// [p, p + (B - 1) * stride + plane) in bytes
inline void extent(const void* p, int64_t B, int64_t stride, int64_t plane, uintptr_t& lo, uintptr_t& hi) {
  lo = (uintptr_t)p;
  hi = lo + (uintptr_t)((B - 1) * stride + plane) * sizeof(float);
}

}  // namespace

// what asrx_logmel and asrx_logmel_pass check alike (a.ws, a.frames and the batch are the entry point's own); fills r
// and a.wtotal
static int lm_check(LmArgs& a, const int32_t* fb_range, LmRanges& r) {
  if (!a.fb || !fb_range || !a.ws || !a.out || a.n_fft < 2 || a.hop < 1 || a.nbins < 1 || a.nbins > a.n_fft ||
      (a.power != 1 && a.power != 2) || a.n_mels < 1)
    return ASRX_ERR_ARG;
  if (a.log_mode < 0 || a.log_mode > 2 || (a.log_mode != 0 && !(a.log_eps > 0.f))) return ASRX_ERR_ARG;
  if (a.istd && !a.mean) return ASRX_ERR_ARG;
  if (a.n_mels > LM_MAXM || a.nbins > 65535) return ASRX_ERR_UNSUPPORTED;
  memset(&r, 0, sizeof(r));
  int64_t total = 0;
  for (int m = 0; m < a.n_mels; ++m) {
    const int32_t lo = fb_range[2 * m], hi = fb_range[2 * m + 1];
    if (lo < 0 || lo > hi || hi > a.nbins) return ASRX_ERR_ARG;
    r.lo[m] = (uint16_t)lo;
    r.hi[m] = (uint16_t)hi;
    r.off[m] = (uint16_t)(total <= LM_WMAX ? total : 0);
    total += hi - lo;
  }
  a.wtotal = total <= LM_WMAX ? (int)total : 0;   // a wider (dense) filterbank is read from memory
  return ASRX_OK;
}

static int lm_launch(const LmArgs& a, const LmRanges& r, int64_t batch, void* stream) {
  const dim3 grid((unsigned)((a.frames + LM_FT - 1) / LM_FT), (unsigned)batch);
  const hipStream_t st = (hipStream_t)stream;
  if (a.n_mels <= 32) hipLaunchKernelGGL(logmel_kernel<4>, grid, dim3(256), 0, st, a, r);
  else if (a.n_mels <= 80) hipLaunchKernelGGL(logmel_kernel<10>, grid, dim3(256), 0, st, a, r);
  else if (a.n_mels <= 128) hipLaunchKernelGGL(logmel_kernel<16>, grid, dim3(256), 0, st, a, r);
  else hipLaunchKernelGGL(logmel_kernel<32>, grid, dim3(256), 0, st, a, r);
  ASRX_CHECK_LAUNCH();
  return ASRX_OK;
}

extern "C" int asrx_logmel(const float* audio, int64_t batch, int64_t samples, int64_t batch_stride,
                           const int32_t* wave_lengths, const float* basis, int32_t n_fft, int32_t hop, int32_t nbins,
                           int32_t power, float scale, const float* fb, const int32_t* fb_range, int32_t n_mels,
                           int32_t log_mode, float log_mul, float log_eps, const float* mean, const float* istd,
                           float pad_value, float* ws, int64_t ws_elems, float* out, int32_t* frame_lengths,
                           void* stream) {
  if (!audio || !basis || batch < 0) return ASRX_ERR_ARG;
  LmArgs a;
  a.ws = ws; a.wave_lengths = wave_lengths; a.fb = fb; a.mean = mean; a.istd = istd; a.out = out;
  a.frame_lengths = frame_lengths; a.frames = 0; a.nbins = nbins; a.n_mels = n_mels; a.n_fft = n_fft;
  a.hop = hop; a.power = power; a.log_mode = log_mode; a.scale = scale; a.log_mul = log_mul; a.log_eps = log_eps;
  a.pad_value = pad_value;
  LmRanges r;
  int rc = lm_check(a, fb_range, r);
  if (rc) return rc;
  if (samples < n_fft) return ASRX_ERR_ARG;
  const int64_t frames = (samples - n_fft) / hop + 1;
  if (batch == 0) return ASRX_OK;
  if (ws_elems < batch * frames * 2 * (int64_t)nbins) return ASRX_ERR_ARG;
  if (batch > 65535 || frames > 0x7fffffffLL) return ASRX_ERR_UNSUPPORTED;
  asrx_gemm_desc d;   // asrx_spectrogram's STFT, unchanged
  memset(&d, 0, sizeof(d));
  d.m = frames; d.n = 2 * (int64_t)nbins; d.k = n_fft;
  d.in_dtype = ASRX_F32;
  d.a = audio; d.lda = hop; d.a_trans = 0;
  d.b = basis; d.ldb = n_fft; d.b_trans = 0;
  d.c = ws; d.ldc = 2 * (int64_t)nbins; d.c_dtype = ASRX_F32;
  d.batch = (int32_t)batch; d.batch_inner = 1;
  d.sa_outer = batch_stride; d.sb_outer = 0; d.sc_outer = frames * 2 * (int64_t)nbins;
  d.alpha = 1.f; d.beta = 0.f; d.splitk = 1;
  rc = asrx_gemm(&d, stream);
  if (rc) return rc;
  a.frames = frames;
  return lm_launch(a, r, batch, stream);
}

extern "C" int asrx_logmel_pass(const float* ws, int64_t batch, int64_t frames, const int32_t* wave_lengths,
                                int32_t n_fft, int32_t hop, int32_t nbins, int32_t power, float scale, const float* fb,
                                const int32_t* fb_range, int32_t n_mels, int32_t log_mode, float log_mul,
                                float log_eps, const float* mean, const float* istd, float pad_value, float* out,
                                int32_t* frame_lengths, void* stream) {
  if (batch < 0 || frames < 1) return ASRX_ERR_ARG;
  LmArgs a;
  a.ws = ws; a.wave_lengths = wave_lengths; a.fb = fb; a.mean = mean; a.istd = istd; a.out = out;
  a.frame_lengths = frame_lengths; a.frames = frames; a.nbins = nbins; a.n_mels = n_mels; a.n_fft = n_fft;
  a.hop = hop; a.power = power; a.log_mode = log_mode; a.scale = scale; a.log_mul = log_mul; a.log_eps = log_eps;
  a.pad_value = pad_value;
  LmRanges r;
  const int rc = lm_check(a, fb_range, r);
  if (rc) return rc;
  if (batch == 0) return ASRX_OK;
  if (batch > 65535 || frames > 0x7fffffffLL) return ASRX_ERR_UNSUPPORTED;
  return lm_launch(a, r, batch, stream);
}

extern "C" int asrx_cmvn(const float* x, float* out, int32_t B, int32_t F, int32_t T, int64_t x_bstride,
                         int64_t out_bstride, const int32_t* lengths, const float* mean, const float* istd,
                         int32_t norm_var, float eps, float pad_value, void* stream) {
  if (!x || !out || B < 0 || F < 1 || T < 1) return ASRX_ERR_ARG;
  if ((((uintptr_t)x | (uintptr_t)out) & 3) != 0) return ASRX_ERR_ARG;
  if (istd && !mean) return ASRX_ERR_ARG;
  if (!mean && norm_var && !(eps > 0.f)) return ASRX_ERR_ARG;
  if (B > 65535) return ASRX_ERR_UNSUPPORTED;
  if (B == 0) return ASRX_OK;
  const int64_t plane = (int64_t)F * T;
  if (B > 1 && (x_bstride < plane || out_bstride < plane)) return ASRX_ERR_ARG;
  if ((const float*)out == x) {   // in place: the same layout
    if (B > 1 && x_bstride != out_bstride) return ASRX_ERR_ARG;
  } else {
    uintptr_t x0, x1, o0, o1;
    extent(x, B, x_bstride, plane, x0, x1);
    extent(out, B, out_bstride, plane, o0, o1);
    if (x0 < o1 && o0 < x1) return ASRX_ERR_ARG;
  }
  CmArgs a;
  a.x = x; a.out = out; a.lengths = lengths; a.mean = mean; a.istd = istd; a.xb = x_bstride; a.ob = out_bstride;
  a.T = T; a.norm_var = norm_var; a.eps = eps; a.pad_value = pad_value;
  hipLaunchKernelGGL(cmvn_kernel, dim3((unsigned)F, (unsigned)B), dim3(256), 0, (hipStream_t)stream, a);
  ASRX_CHECK_LAUNCH();
  return ASRX_OK;
}

extern "C" int asrx_feature_stats(const float* x, int32_t B, int32_t F, int32_t T, int64_t x_bstride,
                                  const int32_t* lengths, double* sum, double* sumsq, int64_t* count, void* stream) {
  if (!x || !sum || !sumsq || !count || B < 0 || F < 1 || T < 1) return ASRX_ERR_ARG;
  if (((uintptr_t)x & 3) != 0 || (((uintptr_t)sum | (uintptr_t)sumsq | (uintptr_t)count) & 7) != 0)
    return ASRX_ERR_ARG;
  if (B == 0) return ASRX_OK;
  if (B > 1 && x_bstride < (int64_t)F * T) return ASRX_ERR_ARG;
  hipLaunchKernelGGL(feature_stats_kernel, dim3((unsigned)F), dim3(256), 0, (hipStream_t)stream, x, (int)B, (int)T,
                     x_bstride, lengths, sum, sumsq, count);
  ASRX_CHECK_LAUNCH();
  return ASRX_OK;
}
