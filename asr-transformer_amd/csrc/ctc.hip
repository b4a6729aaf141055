// CTC (connectionist temporal classification) for the hybrid CTC/attention objective: the negative log-likelihood and
// its gradient with respect to the LOGITS (log-softmax fused, no log-probability tensor), the CTC targets of a
// teacher-forced batch, and best-path decoding.  C-ABI: asrx_ctc_loss, asrx_ctc_workspace_elems, asrx_ctc_targets,
// asrx_ctc_greedy (include/asrx.h).
//
// asrx_ctc_loss is four launches on one stream, everything in the log2 domain (v_exp_f32 / v_log_f32):
//   1. ctc_prep_kernel    blocks [0, B): per sample, validate the target and rank its positions by (label, position)
//                         (the fixed summation order of the occupancy); the other blocks, one wave per (b, t) row:
//                         row maximum and log2(sum 2^((x - max) log2 e)) -> ws.
//   2. ctc_chain_kernel   one wave64 per (sample, direction): wave 0 runs alpha forward in time, wave 1 beta backward.
//                         The sample's 2L + 1 extended states are held as L + 1 (blank, label) PAIRS, lane i owning
//                         the pairs i*KP .. i*KP + KP - 1 (KP = ceil((Lmax + 1) / 64) <= 4, hence L <= 255) in
//                         registers.  Every transition into a pair comes from the pair itself or its neighbour:
//                         alpha needs one value from lane i - 1 (its last label state), beta two from lane i + 1, as
//                         DPP wave shifts — the time loop has no barrier and no LDS round trip.  The emissions of
//                         the next four time steps are loaded while the current four are computed.
//   3. ctc_grad_kernel    one wave per (b, t) row: occupancy of each pair from alpha + beta, the label contributions
//                         written to LDS in rank order so that each distinct label is one contiguous run summed
//                         front to back by the lane of its first occurrence, then one 16-B-vector pass over the row:
//                         dlogits = gs * (softmax - occupancy).
//   4. ctc_finish_kernel  loss = loss_add_scale * loss_add[0] + loss_scale * sum_b w_b nll_b, fixed order.
// No floating-point atomics anywhere: two calls on the same inputs give the same bits.
#include "ctc_common.h"

#include <algorithm>

namespace {

constexpr int CTC_AUX = 260;         // ints per sample: [0, 256) rank | count << 16, [256] L (-1: no alignment can
                                     // exist: bad length or label), [257] input length

struct CtcWs {
  float* stats;   // [B*T][2]: row max, log2 sum
  int* aux;       // [B][CTC_AUX]
  float* nll2;    // [B]: -log2 P
  float* alpha;   // [B*T][128*KP]: pair u at [2u] (blank state 2u), [2u + 1] (label state 2u + 1)
  float* beta;
};

inline int64_t r4(int64_t x) { return (x + 3) & ~(int64_t)3; }
inline int64_t ctc_ws_elems(int64_t B, int64_t T, int max_l) {
  return r4(2 * B * T) + r4(B * CTC_AUX) + r4(B) + 2 * B * T * 128 * ctc_kp(max_l);
}
inline CtcWs ctc_ws(float* ws, int64_t B, int64_t T, int max_l) {
  CtcWs w;
  w.stats = ws;
  w.aux = (int*)(ws + r4(2 * B * T));
  w.nll2 = ws + r4(2 * B * T) + r4(B * CTC_AUX);
  w.alpha = w.nll2 + r4(B);
  w.beta = w.alpha + B * T * 128 * ctc_kp(max_l);
  return w;
}

// ---------------------------------------------------------------------------------------------- 1. prep
__global__ __launch_bounds__(256) void ctc_prep_kernel(const float* __restrict__ logits, int B, int T, int V, int64_t ld,
                                                       const int64_t* __restrict__ targets, int64_t tgt_stride,
                                                       const int32_t* __restrict__ input_lengths,
                                                       const int32_t* __restrict__ target_lengths, int max_l, int blank,
                                                       int vec, float* __restrict__ stats, int* __restrict__ aux) {
  __shared__ int s_tgt[256];
  const int tid = threadIdx.x;
  if ((int)blockIdx.x < B) {
    const int b = blockIdx.x;
    int L = target_lengths[b];
    const bool len_ok = L >= 0 && L <= max_l;
    if (!len_ok) L = 0;
    int bad = 0, lab = -1;
    if (tid < L) {
      const int64_t id = targets[(int64_t)b * tgt_stride + tid];
      bad = id < 0 || id >= V || id == blank;
      lab = bad ? -1 : (int)id;
    }
    s_tgt[tid] = lab;
    bad = __syncthreads_or(bad);
    int word = 0;
    if (tid < L) {
      int less = 0, eq_before = 0, eq_after = 0;
      for (int u = 0; u < L; ++u) {
        const int o = s_tgt[u];
        less += o < lab;
        eq_before += (o == lab) & (u < tid);
        eq_after += (o == lab) & (u > tid);
      }
      word = (less + eq_before) | ((eq_before == 0 ? 1 + eq_after : 0) << 16);
    }
    aux[b * CTC_AUX + tid] = word;
    if (tid == 0) {
      int Tb = input_lengths ? input_lengths[b] : T;
      Tb = Tb < 0 ? 0 : (Tb > T ? T : Tb);   // (written out: clamp_len moves one instruction of this kernel)
      aux[b * CTC_AUX + 256] = (len_ok && !bad) ? L : -1;
      aux[b * CTC_AUX + 257] = Tb;
    }
    return;
  }
  const int l = tid & 63;
  const int64_t r = ((int64_t)blockIdx.x - B) * 4 + (tid >> 6);
  if (r >= (int64_t)B * T) return;
  const float* x = logits + r * ld;
  float mx = -INFINITY, sum = 0.f;
  if (vec) {
    for (int c0 = l * 4; c0 < V; c0 += 256) {
      const f4_t v = *(const f4_t*)(x + c0);
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (c0 + k < V) mx = fmaxf(mx, v[k]);
    }
    mx = wave_max(mx);
    for (int c0 = l * 4; c0 < V; c0 += 256) {
      const f4_t v = *(const f4_t*)(x + c0);
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (c0 + k < V) sum += exp2_raw((v[k] - mx) * kLog2e);
    }
  } else {
    for (int c = l; c < V; c += 64) mx = fmaxf(mx, x[c]);
    mx = wave_max(mx);
    for (int c = l; c < V; c += 64) sum += exp2_raw((x[c] - mx) * kLog2e);
  }
  sum = wave_sum(sum);
  if (l == 0) {
    stats[2 * r] = mx;
    stats[2 * r + 1] = log2_raw(sum);
  }
}

// ---------------------------------------------------------------------------------------------- 2. alpha / beta
constexpr int CTC_U = 4;   // time steps of emissions in flight

template <int KP>
__global__ __launch_bounds__(64) void ctc_chain_kernel(const float* __restrict__ logits, int T, int64_t ld,
                                                       const int64_t* __restrict__ targets, int64_t tgt_stride,
                                                       int blank, CtcWs w, float* __restrict__ nll) {
  const int b = blockIdx.x, dir = blockIdx.y, lane = threadIdx.x;
  const int L = w.aux[b * CTC_AUX + 256], Tb = w.aux[b * CTC_AUX + 257];
  if (L < 0 || Tb <= 0) {   // no alignment (an empty target over no frames has the empty one)
    if (dir == 0 && lane == 0) {
      const float v = (L == 0) ? 0.f : INFINITY;
      nll[b] = v;
      w.nll2[b] = v;
    }
    return;
  }
  // this lane's pairs: label column, validity, and whether the skip transition (s - 2 -> s) exists
  int lab[KP];
  bool vb[KP], vl[KP], skip[KP];
  const int64_t* tg = targets + (int64_t)b * tgt_stride;
#pragma unroll
  for (int q = 0; q < KP; ++q) {
    const int u = lane * KP + q;
    vb[q] = u <= L;
    vl[q] = u < L;
    lab[q] = vl[q] ? (int)tg[u] : blank;
    // alpha: label u from label u - 1; beta: label u from label u + 1
    const int o = dir == 0 ? u - 1 : u + 1;
    skip[q] = vl[q] && o >= 0 && o < L && (int)tg[o] != lab[q];
  }
  float sb[KP], sl[KP];   // log2 alpha (beta) of the blank and label state of each pair at the previous step
#pragma unroll
  for (int q = 0; q < KP; ++q) {
    sb[q] = -INFINITY;
    sl[q] = -INFINITY;
    // virtual step before the first: all mass in blank state 0 (alpha) / blank state 2L (beta)
    if (lane * KP + q == (dir == 0 ? 0 : L)) sb[q] = 0.f;
  }
  float* out = dir == 0 ? w.alpha : w.beta;
  const int64_t row0 = (int64_t)b * T;

  float n_b[CTC_U], n_l[CTC_U][KP], n_m[CTC_U], n_s[CTC_U];
  auto load = [&](int k0) {
#pragma unroll
    for (int i = 0; i < CTC_U; ++i) {
      int k = k0 + i;
      k = k < Tb ? k : Tb - 1;
      const int64_t r = row0 + (dir == 0 ? k : Tb - 1 - k);
      const float* x = logits + r * ld;
      n_b[i] = x[blank];
#pragma unroll
      for (int q = 0; q < KP; ++q) n_l[i][q] = x[lab[q]];
      n_m[i] = w.stats[2 * r];
      n_s[i] = w.stats[2 * r + 1];
    }
  };
  load(0);
  for (int k0 = 0; k0 < Tb; k0 += CTC_U) {
    float c_b[CTC_U], c_l[CTC_U][KP], c_m[CTC_U], c_s[CTC_U];
#pragma unroll
    for (int i = 0; i < CTC_U; ++i) {
      c_b[i] = n_b[i];
      c_m[i] = n_m[i];
      c_s[i] = n_s[i];
#pragma unroll
      for (int q = 0; q < KP; ++q) c_l[i][q] = n_l[i][q];
    }
    load(k0 + CTC_U);
#pragma unroll
    for (int i = 0; i < CTC_U; ++i) {
      if (k0 + i >= Tb) break;
      const int64_t r = row0 + (dir == 0 ? k0 + i : Tb - 1 - (k0 + i));
      const float eb = (c_b[i] - c_m[i]) * kLog2e - c_s[i];
      float nb[KP], nl[KP];
      if (dir == 0) {
        const float in_l = wave_up1(sl[KP - 1], -INFINITY);   // label state of pair u - 1 for q = 0
#pragma unroll
        for (int q = 0; q < KP; ++q) {
          const float pl = q == 0 ? in_l : sl[q - 1];
          const float el = (c_l[i][q] - c_m[i]) * kLog2e - c_s[i];
          nb[q] = vb[q] ? lae2(sb[q], pl) + eb : -INFINITY;
          nl[q] = vl[q] ? lae3(sl[q], sb[q], skip[q] ? pl : -INFINITY) + el : -INFINITY;
        }
      } else {
        const float in_b = wave_down1(sb[0], -INFINITY);      // pair u + 1 for q = KP - 1
        const float in_l = wave_down1(sl[0], -INFINITY);
#pragma unroll
        for (int q = 0; q < KP; ++q) {
          const float xb = q == KP - 1 ? in_b : sb[q + 1 < KP ? q + 1 : q];
          const float xl = q == KP - 1 ? in_l : sl[q + 1 < KP ? q + 1 : q];
          const float el = (c_l[i][q] - c_m[i]) * kLog2e - c_s[i];
          nb[q] = vb[q] ? lae2(sb[q], sl[q]) + eb : -INFINITY;
          nl[q] = vl[q] ? lae3(sl[q], xb, skip[q] ? xl : -INFINITY) + el : -INFINITY;
        }
      }
      f2_t* o = (f2_t*)(out + r * (128 * KP) + lane * (2 * KP));
#pragma unroll
      for (int q = 0; q < KP; ++q) {
        sb[q] = nb[q];
        sl[q] = nl[q];
        o[q] = (f2_t){nb[q], nl[q]};
      }
    }
  }
  if (dir == 0) {   // P = alpha_T(2L) + alpha_T(2L - 1)
    float fb = -INFINITY, fl = -INFINITY;
#pragma unroll
    for (int q = 0; q < KP; ++q) {
      if (q == L % KP) fb = sb[q];
      if (L > 0 && q == (L - 1) % KP) fl = sl[q];
    }
    fb = __shfl(fb, L / KP, 64);
    fl = __shfl(fl, L > 0 ? (L - 1) / KP : 0, 64);
    if (L == 0) fl = -INFINITY;
    const float p2 = lae2(fb, fl);
    if (lane == 0) {
      w.nll2[b] = -p2;
      nll[b] = -p2 * kLn2;
    }
  }
}

// ---------------------------------------------------------------------------------------------- 3. gradient
template <typename OutT> ASRX_DEV void store4(OutT* p, f4_t g);
template <> ASRX_DEV void store4<float>(float* p, f4_t g) { *(f4_t*)p = g; }
template <> ASRX_DEV void store4<bf16_t>(bf16_t* p, f4_t g) {
  *(v2u_t*)p = (v2u_t){pack2bf(g[0], g[1]), pack2bf(g[2], g[3])};
}
template <typename OutT> ASRX_DEV void store1(OutT* p, float g);
template <> ASRX_DEV void store1<float>(float* p, float g) { *p = g; }
template <> ASRX_DEV void store1<bf16_t>(bf16_t* p, float g) { *p = f2bf(g); }

// LDS per wave: cl[256] (label contributions in rank order) then occ[ldp] (occupancy per column)
template <typename OutT>
__global__ __launch_bounds__(256) void ctc_grad_kernel(const float* __restrict__ logits, int B, int T, int V, int64_t ld,
                                                       int ldp, const int64_t* __restrict__ targets, int64_t tgt_stride,
                                                       int blank, int kp, int mean, int zero_infinity, float grad_scale,
                                                       int vec, CtcWs w, OutT* __restrict__ dlogits) {
  extern __shared__ float s_grad[];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  float* cl = s_grad + wv * (256 + ldp);
  float* occ = cl + 256;
  const int64_t rows = (int64_t)B * T;
  const int64_t r = (int64_t)blockIdx.x * 4 + wv;
  const bool row_ok = r < rows;            // (a wave past the end still takes the barriers)
  const int b = row_ok ? (int)(r / T) : 0, t = row_ok ? (int)(r - (int64_t)b * T) : 0;
  const int L = w.aux[b * CTC_AUX + 256], Tb = w.aux[b * CTC_AUX + 257];
  const float nll2 = w.nll2[b];
  const bool feasible = L >= 0 && nll2 < INFINITY;
  const bool live = row_ok && t < Tb && feasible;
  const float* x = logits + r * ld;
  float mx = 0.f, l2s = 0.f;
  int auxw[4], labs[4];
  if (live) {
    mx = w.stats[2 * r];
    l2s = w.stats[2 * r + 1];
    for (int c = lane; c < ldp; c += 64) occ[c] = 0.f;
    const float eb = (x[blank] - mx) * kLog2e - l2s;
    float bsum = 0.f;
    const float* al = w.alpha + r * (128 * kp) + lane * (2 * kp);
    const float* be = w.beta + r * (128 * kp) + lane * (2 * kp);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      auxw[q] = 0;
      labs[q] = 0;
      const int u = lane * kp + q;
      if (q < kp && u <= L) {
        const f2_t a = *(const f2_t*)(al + 2 * q), bt = *(const f2_t*)(be + 2 * q);
        bsum += exp2_raw(a[0] + bt[0] - eb + nll2);
        if (u < L) {
          const int lab = (int)targets[(int64_t)b * tgt_stride + u];   // validated by the prep launch
          const float el = (x[lab] - mx) * kLog2e - l2s;
          const int aw = w.aux[b * CTC_AUX + u];
          cl[aw & 0xffff] = exp2_raw(a[1] + bt[1] - el + nll2);
          auxw[q] = aw;
          labs[q] = lab;
        }
      }
    }
    bsum = wave_sum(bsum);
    if (lane == 0) occ[blank] = bsum;
  }
  __syncthreads();
  if (live) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int cnt = auxw[q] >> 16;
      if (cnt > 0) {   // first occurrence of its label: the label's run, front to back
        const float* run = cl + (auxw[q] & 0xffff);
        float s = run[0];
        for (int k = 1; k < cnt; ++k) s += run[k];
        occ[labs[q]] = s;
      }
    }
  }
  __syncthreads();
  if (!row_ok) return;
  OutT* g = dlogits + r * ld;
  const bool nan_row = t < Tb && !feasible && !zero_infinity;
  float gs = grad_scale;
  if (mean) gs = gs / ((float)B * (float)(L > 1 ? L : 1));
  const float dead = nan_row ? __builtin_nanf("") : 0.f;
  if (vec) {
    for (int c0 = lane * 4; c0 < (int)ld; c0 += 256) {
      f4_t o = {0.f, 0.f, 0.f, 0.f};
      if (c0 < V) {
        const f4_t v = *(const f4_t*)(x + c0);
#pragma unroll
        for (int k = 0; k < 4; ++k)
          if (c0 + k < V) o[k] = live ? gs * (exp2_raw((v[k] - mx) * kLog2e - l2s) - occ[c0 + k]) : dead;
      }
      store4<OutT>(g + c0, o);
    }
  } else {
    for (int c = lane; c < (int)ld; c += 64) {
      float o = 0.f;
      if (c < V) o = live ? gs * (exp2_raw((x[c] - mx) * kLog2e - l2s) - occ[c]) : dead;
      store1<OutT>(g + c, o);
    }
  }
}

// ---------------------------------------------------------------------------------------------- 4. loss
__global__ __launch_bounds__(64) void ctc_finish_kernel(const float* __restrict__ nll, int B, const int* __restrict__ aux,
                                                        int mean, int zero_infinity, const float* __restrict__ loss_add,
                                                        float loss_add_scale, float loss_scale,
                                                        float* __restrict__ loss) {
  const int lane = threadIdx.x;
  float s = 0.f;
  for (int b = lane; b < B; b += 64) {
    float v = nll[b];
    if (zero_infinity && v == INFINITY) v = 0.f;
    if (mean) {
      const int L = aux[b * CTC_AUX + 256];
      v = v / (float)(L > 1 ? L : 1);
    }
    s += v;
  }
  s = wave_sum(s);
  if (mean) s = s / (float)B;
  if (lane == 0) {
    float out = loss_scale * s;
    if (loss_add) out = __builtin_fmaf(loss_add_scale, loss_add[0], out);
    loss[0] = out;
  }
}

// ---------------------------------------------------------------------------------------------- targets
struct CtcDrop { int64_t id[4]; int n; };

__global__ __launch_bounds__(64) void ctc_targets_kernel(const int64_t* __restrict__ text, int64_t ld_text,
                                                         const float* __restrict__ mask, int64_t ld_mask, int n,
                                                         CtcDrop drop, int64_t blank, int64_t* __restrict__ targets,
                                                         int64_t ld_tgt, int32_t* __restrict__ target_lengths) {
  const int b = blockIdx.x, lane = threadIdx.x;
  int base = 0;
  for (int p0 = 0; p0 < n; p0 += 64) {
    const int p = p0 + lane;
    bool keep = false;
    int64_t tok = 0;
    if (p < n) {
      tok = text[(int64_t)b * ld_text + p];
      keep = mask[(int64_t)b * ld_mask + p] >= 1.f;
      for (int k = 0; k < drop.n; ++k) keep = keep && tok != drop.id[k];
    }
    const uint64_t m = __ballot(keep);
    if (keep) targets[(int64_t)b * ld_tgt + base + __popcll(m & ((1ull << lane) - 1))] = tok;
    base += __popcll(m);
  }
  for (int p = base + lane; p < n; p += 64) targets[(int64_t)b * ld_tgt + p] = blank;
  if (lane == 0) target_lengths[b] = base;
}

// ---------------------------------------------------------------------------------------------- best path
__global__ __launch_bounds__(1024) void ctc_greedy_kernel(const float* __restrict__ logits, int T, int V, int64_t ld,
                                                          const int32_t* __restrict__ input_lengths, int blank,
                                                          int64_t* __restrict__ tok, int32_t* __restrict__ len) {
  extern __shared__ int s_am[];   // [T] per-frame arg-max
  const int b = blockIdx.x, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int Tb = clamp_len(input_lengths ? input_lengths[b] : T, T);
  for (int t = wv; t < Tb; t += 16) {
    const float* x = logits + ((int64_t)b * T + t) * ld;
    float mx = -INFINITY;
    int am = V;   // first index of the maximum; a row of NaN / -inf only gives 0 (asrx_greedy_argmax's rule)
    for (int c = lane; c < V; c += 64) {
      const float v = x[c];
      if (v > mx || (am == V && !(v < mx))) { mx = v; am = c; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float om = __shfl_xor(mx, o, 64);
      const int oa = __shfl_xor(am, o, 64);
      if (om > mx || (om == mx && oa < am)) { mx = om; am = oa; }
    }
    if (lane == 0) s_am[t] = am < V ? am : 0;
  }
  __syncthreads();
  if (wv != 0) return;
  int64_t* out = tok + (int64_t)b * T;
  int base = 0;
  for (int t0 = 0; t0 < Tb; t0 += 64) {
    const int t = t0 + lane;
    bool keep = false;
    int a = 0;
    if (t < Tb) {
      a = s_am[t];
      keep = a != blank && (t == 0 || a != s_am[t - 1]);
    }
    const uint64_t m = __ballot(keep);
    if (keep) out[base + __popcll(m & ((1ull << lane) - 1))] = a;
    base += __popcll(m);
  }
  for (int p = base + lane; p < T; p += 64) out[p] = blank;
  if (lane == 0) len[b] = base;
}

}  // namespace

extern "C" int64_t asrx_ctc_workspace_elems(int32_t B, int32_t T, int32_t max_target_len) {
  if (B <= 0 || T <= 0 || max_target_len < 0 || max_target_len > CTC_MAXL) return -1;
  return ctc_ws_elems(B, T, max_target_len);
}

extern "C" int asrx_ctc_loss(const float* logits, int32_t B, int32_t T, int32_t V, int64_t ld, const int64_t* targets,
                             int64_t tgt_stride, const int32_t* input_lengths, const int32_t* target_lengths,
                             int32_t max_target_len, int32_t blank, int32_t reduction, int32_t zero_infinity,
                             float grad_scale, float* nll, float* loss, void* dlogits, int32_t dlogits_dtype,
                             const float* loss_add, float loss_add_scale, float loss_scale, float* ws,
                             int64_t ws_elems, void* stream) {
  // (these two stand before the first ASRX_ERR_UNSUPPORTED of the shared checks, whose earlier ones return
  // ASRX_ERR_ARG as well: a call that breaks several rules gets the same code wherever among those they stand)
  if (reduction != ASRX_CTC_SUM && reduction != ASRX_CTC_MEAN) return ASRX_ERR_ARG;
  if (dlogits && dlogits_dtype != ASRX_BF16 && dlogits_dtype != ASRX_F32) return ASRX_ERR_ARG;
  const bool own_ok = logits && target_lengths && nll && loss && ws && ((uintptr_t)ws & 15) == 0 &&
                      ws_elems >= ctc_ws_elems(B, T, std::min(max_target_len, CTC_MAXL));   // (beyond: refused before)
  const int err = ctc_check_target_args(B, T, V, ld, targets, tgt_stride, max_target_len, blank, own_ok);
  if (err != ASRX_OK) return err;
  if (ld > 8192) return ASRX_ERR_UNSUPPORTED;   // the gradient's per-wave occupancy row lives in LDS
  hipStream_t st = (hipStream_t)stream;
  const CtcWs w = ctc_ws(ws, B, T, max_target_len);
  const int kp = ctc_kp(max_target_len);
  const int64_t rows = (int64_t)B * T;
  const int mean = reduction == ASRX_CTC_MEAN;
  const int vec_in = ld % 4 == 0 && ((uintptr_t)logits & 15) == 0;
  const int64_t* tg = ctc_targets_or_dummy(targets);

  hipLaunchKernelGGL(ctc_prep_kernel, dim3((unsigned)(B + (rows + 3) / 4)), dim3(256), 0, st, logits, B, T, V, ld, tg,
                     tgt_stride, input_lengths, target_lengths, max_target_len, blank, vec_in, w.stats, w.aux);
  ASRX_CHECK_LAUNCH();
  const dim3 cgrid((unsigned)B, 2);
  ctc_dispatch_kp(kp, [&](auto kpc) {
    hipLaunchKernelGGL(ctc_chain_kernel<decltype(kpc)::value>, cgrid, dim3(64), 0, st, logits, T, ld, tg, tgt_stride,
                       blank, w, nll);
  });
  ASRX_CHECK_LAUNCH();
  if (dlogits) {
    const int ldp = (int)((ld + 3) & ~(int64_t)3);
    const size_t shm = sizeof(float) * 4 * (256 + ldp);
    const unsigned grid = (unsigned)((rows + 3) / 4);
    if (dlogits_dtype == ASRX_F32) {
      const int vec = vec_in && ((uintptr_t)dlogits & 15) == 0;
      hipLaunchKernelGGL(ctc_grad_kernel<float>, dim3(grid), dim3(256), shm, st, logits, B, T, V, ld, ldp, tg,
                         tgt_stride, blank, kp, mean, zero_infinity, grad_scale, vec, w, (float*)dlogits);
    } else {
      const int vec = vec_in && ((uintptr_t)dlogits & 7) == 0;
      hipLaunchKernelGGL(ctc_grad_kernel<bf16_t>, dim3(grid), dim3(256), shm, st, logits, B, T, V, ld, ldp, tg,
                         tgt_stride, blank, kp, mean, zero_infinity, grad_scale, vec, w, (bf16_t*)dlogits);
    }
    ASRX_CHECK_LAUNCH();
  }
  hipLaunchKernelGGL(ctc_finish_kernel, dim3(1), dim3(64), 0, st, nll, B, w.aux, mean, zero_infinity, loss_add,
                     loss_add_scale, loss_scale, loss);
  ASRX_CHECK_LAUNCH();
  return ASRX_OK;
}

extern "C" int asrx_ctc_targets(const int64_t* text, int64_t ld_text, const float* mask, int64_t ld_mask, int32_t B,
                                int32_t n, const int64_t* drop, int32_t ndrop, int64_t blank, int64_t* targets,
                                int64_t ld_targets, int32_t* target_lengths, void* stream) {
  if (!text || !mask || !targets || !target_lengths || B <= 0 || n <= 0) return ASRX_ERR_ARG;
  if (ld_text < n || ld_mask < n || ld_targets < n || ndrop < 0 || ndrop > 4 || (ndrop > 0 && !drop)) return ASRX_ERR_ARG;
  CtcDrop d;
  d.n = ndrop;
  for (int k = 0; k < 4; ++k) d.id[k] = k < ndrop ? drop[k] : 0;
  hipLaunchKernelGGL(ctc_targets_kernel, dim3((unsigned)B), dim3(64), 0, (hipStream_t)stream, text, ld_text, mask,
                     ld_mask, n, d, blank, targets, ld_targets, target_lengths);
  ASRX_CHECK_LAUNCH();
  return ASRX_OK;
}

extern "C" int asrx_ctc_greedy(const float* logits, int32_t B, int32_t T, int32_t V, int64_t ld,
                               const int32_t* input_lengths, int32_t blank, int64_t* tok, int32_t* len, void* stream) {
  if (!logits || !tok || !len || B <= 0 || T <= 0 || V <= 0 || ld < V || blank < 0 || blank >= V) return ASRX_ERR_ARG;
  if (T > 15360) return ASRX_ERR_UNSUPPORTED;   // the per-frame arg-max of a sample is held in LDS (60 KiB)
  hipLaunchKernelGGL(ctc_greedy_kernel, dim3((unsigned)B), dim3(1024), sizeof(int) * T, (hipStream_t)stream, logits, T,
                     V, ld, input_lengths, blank, tok, len);
  ASRX_CHECK_LAUNCH();
  return ASRX_OK;
}
