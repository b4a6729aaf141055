// CTC prefix scoring for joint CTC/attention beam search (Watanabe et al. 2017): every beam hypothesis g carries the
// forward state of the CTC head over the utterance's frames, and each decode step asks for the prefix probability
// psi(g.c) of every continuation c.  C-ABI: asrx_ctc_prefix_init, asrx_ctc_prefix_score, asrx_ctc_prefix_advance
// (include/asrx.h); the selection that consumes the scores is asrx_beam_step_joint (decode.hip).
//
// With y_t(v) the head's softmax, gn_t(g) / gb_t(g) the probability of all paths over frames 0..t that collapse to g
// and end in a non-blank / in the blank, and h = g.c:
//   phi_t   = gb_{t-1}(g) + (c != last(g) ? gn_{t-1}(g) : 0)
//   psi(h)  = sum_t phi_t y_t(c)
//   gn_t(h) = (gn_{t-1}(h) + phi_t) y_t(c),   gb_t(h) = (gb_{t-1}(h) + gn_{t-1}(h)) y_t(blank)
// (t = -1: gb = 1 for the empty prefix, everything else 0).  psi(g.c) needs g's state only, in two variants per frame,
// so the state of a slot is stored as the PAIR (log2(gn_t + gb_t), log2 gb_t): scoring all V continuations of the W
// hypotheses of a sample is a log-semiring product [W x T] . [T x V] (prefix_score_kernel, no recursion), and only
// the W survivors of the selection run the serial chain over t (prefix_advance_kernel).
//
// Everything is fp32 in the log2 domain (v_exp_f32 / v_log_f32), every log-sum-exp max-subtracted; the scores leave
// in natural-log units.  No atomics, fixed summation orders: the same inputs give the same bits.
#include "ctc_common.h"

namespace {

constexpr int PFX_MAXW = 16;
constexpr int PFX_SLICES = 4;   // waves of a scoring workgroup: each sweeps a quarter of the frames

// running (max, sum of 2^(x - max)) of a log-sum-exp: one exponential per term
ASRX_DEV void lse_push(float& m, float& s, float x) {
  float d = x - m;
  if (d != d) d = -INFINITY;   // -inf - -inf: nothing to add
  const float e = exp2_raw(-fabsf(d));
  s = d > 0.f ? __builtin_fmaf(s, e, 1.f) : s + e;
  m = fmaxf(m, x);
}
ASRX_DEV void lse_merge(float& m, float& s, float m2, float s2) {
  const float hi = fmaxf(m, m2);
  const float hs = hi == -INFINITY ? 0.f : hi;
  s = s * exp2_raw(m - hs) + s2 * exp2_raw(m2 - hs);
  m = hi;
}

// ---------------------------------------------------------------------------------------------- init
// one wave per (b, t) row: logp[r][c] = log2 softmax(logits[r])[c]
__global__ __launch_bounds__(256) void prefix_logp_kernel(const float* __restrict__ logits, int64_t rows, int V,
                                                          int64_t ld, float* __restrict__ logp) {
  const int lane = threadIdx.x & 63;
  const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= rows) return;
  const float* x = logits + r * ld;
  float mx = -INFINITY, sum = 0.f;
  for (int c = lane; c < V; c += 64) mx = fmaxf(mx, x[c]);
  mx = wave_max(mx);
  for (int c = lane; c < V; c += 64) sum += exp2_raw((x[c] - mx) * kLog2e);
  const float l2s = log2_raw(wave_sum(sum));
  float* o = logp + r * V;
  for (int c = lane; c < V; c += 64) o[c] = (x[c] - mx) * kLog2e - l2s;
}

// one wave per sample: the frame count, and the empty prefix's state (gn = 0, gb_t = prod_{u <= t} y_u(blank)) for
// all W slots
__global__ __launch_bounds__(64) void prefix_root_kernel(const float* __restrict__ logp, int W, int T, int V,
                                                         const int32_t* __restrict__ input_lengths, int blank,
                                                         int32_t* __restrict__ frames, float* __restrict__ state,
                                                         float* __restrict__ logpsi, int32_t* __restrict__ last) {
  const int b = blockIdx.x, lane = threadIdx.x;
  const int Tb = clamp_len(input_lengths ? input_lengths[b] : T, T);
  if (lane == 0) frames[b] = Tb;
  if (lane < W) {
    logpsi[b * W + lane] = 0.f;
    last[b * W + lane] = -1;
  }
  const float* lp = logp + (int64_t)b * T * V + blank;
  float carry = 0.f;
  for (int t0 = 0; t0 < T; t0 += 64) {
    const int t = t0 + lane;
    float v = t < Tb ? lp[(int64_t)t * V] : 0.f;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {   // inclusive scan over the 64 frames of the chunk
      const float u = __shfl_up(v, o, 64);
      if (lane >= o) v += u;
    }
    v += carry;
    carry = __shfl(v, 63, 64);
    if (t < T) {
      const float g = t < Tb ? v : -INFINITY;
      for (int w = 0; w < W; ++w) ((f2_t*)state)[((int64_t)(b * W + w)) * T + t] = (f2_t){g, g};
    }
  }
}

// ---------------------------------------------------------------------------------------------- score
// Workgroup (column chunk of 64, sample): lane = column, wave = a quarter of the sample's frames.  Each wave stages
// the phi pairs of its W hypotheses for 32 frames at a time in LDS (coalesced 8-byte loads; the t = -1 values stand
// in front of frame 0) and reads them back as broadcasts, so the inner loop touches global memory only for the
// column's log-probabilities: a sample's table is read once per step, not W times.  The W running (max, sum) pairs
// of a column stay in registers; the four partial pairs meet in LDS in wave order.
constexpr int PFX_CHUNK = 32;

template <int WT>
__global__ __launch_bounds__(64 * PFX_SLICES) void prefix_score_kernel(
    const float* __restrict__ logp, const int32_t* __restrict__ frames, int W, int T, int V, int blank, int eos,
    const float* __restrict__ state, const float* __restrict__ logpsi, const int32_t* __restrict__ last,
    float* __restrict__ delta, int64_t ldd) {
  __shared__ f2_t s_phi[PFX_SLICES][WT][PFX_CHUNK];
  __shared__ f2_t s_part[PFX_SLICES - 1][WT][64];
  const int lane = threadIdx.x & 63;
  const int slice = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int b = blockIdx.y;
  const int c = blockIdx.x * 64 + lane;
  const int cc = c < V ? c : V - 1;   // lanes past V read column V - 1 and store nothing
  const int Tb = clamp_len(frames[b], T);
  const int per = (Tb + PFX_SLICES - 1) / PFX_SLICES;
  const int t0 = slice * per;
  const int t1 = t0 + per < Tb ? t0 + per : Tb;
  const int64_t slot0 = (int64_t)b * W;

  float m[WT], s[WT];
  bool same[WT];
  int root[WT];
#pragma unroll
  for (int w = 0; w < WT; ++w) {
    m[w] = -INFINITY;
    s[w] = 0.f;
    const int l = w < W ? last[slot0 + w] : -1;
    same[w] = cc == l;
    root[w] = l < 0;
  }
  const float* lp = logp + (int64_t)b * T * V + cc;
  const f2_t* st2 = (const f2_t*)state;
  // every wave runs the same number of rounds (the barriers), a short or empty slice with fewer or no frames in them
  for (int k0 = 0; k0 < per; k0 += PFX_CHUNK) {
    const int tc = t0 + k0;
    const int n = t1 - tc < PFX_CHUNK ? t1 - tc : PFX_CHUNK;   // (<= 0: nothing left in this slice)
#pragma unroll
    for (int e = lane; e < WT * PFX_CHUNK; e += 64) {   // (rows w >= W hold -inf: the loop below has no branch)
      const int w = e / PFX_CHUNK, i = e % PFX_CHUNK, t = tc + i;
      f2_t v = {-INFINITY, -INFINITY};
      if (i < n && w < W) {
        if (t > 0) {
          v = st2[(slot0 + w) * T + (t - 1)];
        } else if (last[slot0 + w] < 0) {   // gb_{-1} = 1 for the empty prefix only
          v = (f2_t){0.f, 0.f};
        }
      }
      s_phi[slice][w][i] = v;
    }
    __syncthreads();
#pragma unroll 4
    for (int i = 0; i < n; ++i) {
      const float y = lp[(int64_t)(tc + i) * V];
#pragma unroll
      for (int w = 0; w < WT; ++w) {
        const f2_t p = s_phi[slice][w][i];
        lse_push(m[w], s[w], (same[w] ? p[1] : p[0]) + y);
      }
    }
    __syncthreads();
  }
  if (slice > 0) {
#pragma unroll
    for (int w = 0; w < WT; ++w) s_part[slice - 1][w][lane] = (f2_t){m[w], s[w]};
  }
  __syncthreads();
  if (slice > 0 || c >= V) return;
#pragma unroll
  for (int k = 0; k < PFX_SLICES - 1; ++k) {
#pragma unroll
    for (int w = 0; w < WT; ++w) {
      const f2_t p = s_part[k][w][lane];
      lse_merge(m[w], s[w], p[0], p[1]);
    }
  }
#pragma unroll
  for (int w = 0; w < WT; ++w) {
    if (w < W) {
      const float base = logpsi[slot0 + w];
      float v = m[w] + log2_raw(s[w]);   // (nothing summed: -inf + -inf)
      if (c == eos) v = Tb > 0 ? state[((slot0 + w) * T + (Tb - 1)) * 2] : (root[w] ? 0.f : -INFINITY);
      float d = (v - base) * kLn2;
      if (c == blank || base == -INFINITY || v == -INFINITY) d = -INFINITY;
      delta[(slot0 + w) * ldd + c] = d;
    }
  }
}

// ---------------------------------------------------------------------------------------------- advance
// One wave per slot.  A slot whose parent had finished, or that took EOS, copies the parent's state; any other runs
// the chain over t < T_b.  Lane i stages frame t0 + i of a 64-frame chunk (phi, log2 y(c), log2 y(blank)) while the
// previous chunk's chain runs; the chain itself is wave-uniform (v_readlane of the staged operands), lane i keeps
// step i's result and the chunk is stored as one coalesced row.  psi(h) is a plain reduction of the staged terms.
__global__ __launch_bounds__(64) void prefix_advance_kernel(
    const float* __restrict__ logp, const int32_t* __restrict__ frames, int W, int T, int V, int blank, int eos,
    const int32_t* __restrict__ parent, const int64_t* __restrict__ tok, const uint8_t* __restrict__ fin_prev,
    const float* __restrict__ state_in, const float* __restrict__ logpsi_in, const int32_t* __restrict__ last_in,
    float* __restrict__ state_out, float* __restrict__ logpsi_out, int32_t* __restrict__ last_out) {
  const int slot = blockIdx.x, lane = threadIdx.x;
  const int b = slot / W;
  int p = parent[slot];
  p = clamp_len(p, W - 1);
  const int64_t ps = (int64_t)b * W + p;
  const int64_t tk = tok[slot];
  const int c = tk < 0 ? 0 : (tk >= V ? V - 1 : (int)tk);
  const f2_t* src = (const f2_t*)state_in + ps * T;
  f2_t* dst = (f2_t*)state_out + (int64_t)slot * T;
  if (fin_prev[ps] != 0 || c == eos) {
    for (int t = lane; t < T; t += 64) dst[t] = src[t];
    if (lane == 0) {
      logpsi_out[slot] = logpsi_in[ps];
      last_out[slot] = last_in[ps];
    }
    return;
  }
  const int Tb = clamp_len(frames[b], T);
  const int lst = last_in[ps];
  const bool same = c == lst;
  const float phi0 = lst < 0 ? 0.f : -INFINITY;
  const float* lp = logp + (int64_t)b * T * V;

  float n_phi, n_yc, n_yb;
  auto load = [&](int t) {
    n_phi = -INFINITY;
    n_yc = 0.f;
    n_yb = 0.f;
    if (t < Tb) {
      if (t == 0) {
        n_phi = phi0;
      } else {
        const f2_t g = src[t - 1];
        n_phi = same ? g[1] : g[0];
      }
      n_yc = lp[(int64_t)t * V + c];
      n_yb = lp[(int64_t)t * V + blank];
    }
  };
  float gn = -INFINITY, gb = -INFINITY;   // log2 gn_{t-1}(h), log2 gb_{t-1}(h)
  float pm = -INFINITY, psum = 0.f;       // this lane's share of psi(h)
  load(lane);
  for (int t0 = 0; t0 < Tb; t0 += 64) {
    const float phi = n_phi, yc = n_yc, yb = n_yb;
    load(t0 + 64 + lane);
    lse_push(pm, psum, phi + yc);
    float my_n = -INFINITY, my_b = -INFINITY;
    // (a last chunk of fewer than 64 frames runs its tail on phi = -inf, y = 1: nothing of it is stored)
#pragma unroll 8
    for (int i = 0; i < 64; ++i) {
      const float ph = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(phi), i));
      const float ec = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(yc), i));
      const float eb = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(yb), i));
      const float nn = lae2(gn, ph) + ec;
      const float nb = lae2(gb, gn) + eb;
      gn = nn;
      gb = nb;
      if (lane == i) {
        my_n = nn;
        my_b = nb;
      }
    }
    if (t0 + lane < Tb) dst[t0 + lane] = (f2_t){lae2(my_n, my_b), my_b};
  }
  for (int t = Tb + lane; t < T; t += 64) dst[t] = (f2_t){-INFINITY, -INFINITY};
  const float hi = wave_max(pm);
  const float hs = hi == -INFINITY ? 0.f : hi;
  const float tot = wave_sum(psum * exp2_raw(pm - hs));
  if (lane == 0) {
    logpsi_out[slot] = hi + log2_raw(tot);
    last_out[slot] = c;
  }
}

bool overlap(const void* a, const void* b, int64_t bytes) {
  const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
  return x < y ? x + (uintptr_t)bytes > y : y + (uintptr_t)bytes > x;
}

}  // namespace

extern "C" int asrx_ctc_prefix_init(const float* logits, int32_t B, int32_t W, int32_t T, int32_t V, int64_t ld,
                                    const int32_t* input_lengths, int32_t blank, float* logp, int32_t* frames,
                                    float* state, float* logpsi, int32_t* last, void* stream) {
  if (B < 0 || T <= 0 || V <= 0 || ld < V || W < 1 || W > PFX_MAXW || blank < 0 || blank >= V) return ASRX_ERR_ARG;
  if (!logits || !logp || !frames || !state || !logpsi || !last || ((uintptr_t)state & 7) != 0) return ASRX_ERR_ARG;
  if ((int64_t)B * T > 0x7fffffffLL / 4 || (int64_t)B * W > 0x7fffffffLL) return ASRX_ERR_UNSUPPORTED;
  if (B == 0) return ASRX_OK;
  hipStream_t st = (hipStream_t)stream;
  const int64_t rows = (int64_t)B * T;
  hipLaunchKernelGGL(prefix_logp_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, st, logits, rows, (int)V, ld,
                     logp);
  ASRX_CHECK_LAUNCH();
  hipLaunchKernelGGL(prefix_root_kernel, dim3((unsigned)B), dim3(64), 0, st, (const float*)logp, (int)W, (int)T,
                     (int)V, input_lengths, (int)blank, frames, state, logpsi, last);
  ASRX_CHECK_LAUNCH();
  return ASRX_OK;
}

extern "C" int asrx_ctc_prefix_score(const float* logp, const int32_t* frames, int32_t B, int32_t W, int32_t T,
                                     int32_t V, int32_t blank, int32_t eos, const float* state, const float* logpsi,
                                     const int32_t* last, float* delta, int64_t ld_delta, void* stream) {
  if (B < 0 || T <= 0 || V <= 0 || ld_delta < V || W < 1 || W > PFX_MAXW) return ASRX_ERR_ARG;
  if (blank < 0 || blank >= V || eos < 0 || eos >= V || eos == blank) return ASRX_ERR_ARG;
  if (!logp || !frames || !state || !logpsi || !last || !delta) return ASRX_ERR_ARG;
  if (B > 65535 || (int64_t)B * W > 0x7fffffffLL) return ASRX_ERR_UNSUPPORTED;
  if (B == 0) return ASRX_OK;
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)((V + 63) / 64), (unsigned)B), block(64 * PFX_SLICES);
#define PFX_SCORE(WT)                                                                                              \
  hipLaunchKernelGGL(prefix_score_kernel<WT>, grid, block, 0, st, logp, frames, (int)W, (int)T, (int)V, (int)blank, \
                     (int)eos, state, logpsi, last, delta, ld_delta)
  if (W == 1) PFX_SCORE(1);
  else if (W == 2) PFX_SCORE(2);
  else if (W <= 4) PFX_SCORE(4);
  else if (W <= 8) PFX_SCORE(8);
  else PFX_SCORE(16);
#undef PFX_SCORE
  ASRX_CHECK_LAUNCH();
  return ASRX_OK;
}

extern "C" int asrx_ctc_prefix_advance(const float* logp, const int32_t* frames, int32_t B, int32_t W, int32_t T,
                                       int32_t V, int32_t blank, int32_t eos, const int32_t* parent,
                                       const int64_t* tok, const uint8_t* fin_prev, const float* state_in,
                                       const float* logpsi_in, const int32_t* last_in, float* state_out,
                                       float* logpsi_out, int32_t* last_out, void* stream) {
  if (B < 0 || T <= 0 || V <= 0 || W < 1 || W > PFX_MAXW) return ASRX_ERR_ARG;
  if (blank < 0 || blank >= V || eos < 0 || eos >= V || eos == blank) return ASRX_ERR_ARG;
  if (!logp || !frames || !parent || !tok || !fin_prev || !state_in || !logpsi_in || !last_in || !state_out ||
      !logpsi_out || !last_out)
    return ASRX_ERR_ARG;
  if ((((uintptr_t)state_in | (uintptr_t)state_out) & 7) != 0) return ASRX_ERR_ARG;
  if ((int64_t)B * W > 0x7fffffffLL) return ASRX_ERR_UNSUPPORTED;
  if (B == 0) return ASRX_OK;
  const int64_t R = (int64_t)B * W;
  if (overlap(state_in, state_out, R * T * 2 * (int64_t)sizeof(float)) ||
      overlap(logpsi_in, logpsi_out, R * (int64_t)sizeof(float)) ||
      overlap(last_in, last_out, R * (int64_t)sizeof(int32_t)))
    return ASRX_ERR_ARG;
  hipLaunchKernelGGL(prefix_advance_kernel, dim3((unsigned)R), dim3(64), 0, (hipStream_t)stream, logp, frames, (int)W,
                     (int)T, (int)V, (int)blank, (int)eos, parent, tok, fin_prev, state_in, logpsi_in, last_in,
                     state_out, logpsi_out, last_out);
  ASRX_CHECK_LAUNCH();
  return ASRX_OK;
}
