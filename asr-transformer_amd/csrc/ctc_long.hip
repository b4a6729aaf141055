// CTC loss and forced alignment for transcripts of up to 4095 labels.  C-ABI: asrx_ctc_loss_long,
// asrx_ctc_long_workspace_elems, asrx_ctc_align_long, asrx_ctc_align_long_workspace_words (include/asrx.h).
//
// The math, the launches and the outputs are those of ctc.hip and ctc_align.hip; what changes is who holds the
// sample's L + 1 (blank, label) pairs.  There one wave64 holds them, at most 4 per lane, hence L <= 255.  Here a
// WORKGROUP of NW = ceil((Lmax + 1) / 256) waves (1 .. 16) does, thread i of the workgroup owning pairs 4i .. 4i + 3:
//   - within a wave the neighbour's value still comes by the DPP shift (wave_up1 / wave_down1), whose fill operand is
//     what lane 0 (lane 63) receives;
//   - across a wave seam that fill comes from LDS: after every frame lane 63 of each wave publishes its last label
//     state and lane 0 its first blank and label state into the slot set of the NEXT frame's parity, and one
//     __syncthreads() per frame separates a frame's writes from the next frame's reads (the slots a frame writes were
//     last read one barrier earlier);
//   - the skip flag of a pair needs the neighbouring pair's label, which is read from the targets, not shifted.
// BARRIER UNIFORMITY: every wave of a workgroup executes the same barriers.  The only exits before or between
// barriers are taken on values every thread of the workgroup reads from the same address (the sample's L, T_b and
// feasibility); the time loops run T_b trips in every wave, whether or not the wave owns a live pair.
//
// Loss: four launches (prep, chain, gradient, finish) as in ctc.hip, log2 domain, alpha / beta rows of 512 * NW floats
// in the workspace; the gradient kernel takes one workgroup of 256 threads per (b, t) row over up to 4096 pairs.
// Alignment: two launches as in ctc_align.hip; the renormalising maximum is a workgroup maximum that rides on the
// frame's one barrier; the backpointers (3 bits per pair, one 16-bit word per thread and frame, [frame][64 * NW])
// always live in the workspace and the backtrace is a plain dependent walk over them by wave 0.
// No atomics, fixed orders: the same inputs give the same bits.  Every output element is written by every call.
#include "ctc_common.h"

#include <algorithm>

namespace {

constexpr int CL_MAXL = ASRX_CTC_LONG_MAX_TARGET;   // L + 1 <= 4096 pairs = 1024 threads x 4
constexpr int CL_KP = 4;                            // pairs per thread
constexpr int CL_MAXNW = 16;                        // waves per workgroup
constexpr int CL_SLOTS = CL_MAXL + 1;
constexpr int CL_AUX = CL_SLOTS + 4;   // ints per sample: [0, 4096) rank | count << 16, [4096] L (-1: no alignment
                                       // can exist: bad length or label), [4097] input length
constexpr int CL_U = 4;                // time steps of emissions in flight

inline int cl_nw(int max_l) { return max_l / 256 + 1; }   // = ceil((max_l + 1) / 256) for max_l >= 0

// ctc_check_target_args with this file's bound, in the same order
inline int cl_check_target_args(int32_t B, int32_t T, int32_t V, int64_t ld, const int64_t* targets, int64_t tgt_stride,
                                int32_t max_target_len, int32_t blank, bool own_ok) {
  if (B <= 0 || T <= 0 || V <= 0 || ld < V || max_target_len < 0 || tgt_stride < 0) return ASRX_ERR_ARG;
  if (blank < 0 || blank >= V) return ASRX_ERR_ARG;
  if (max_target_len > CL_MAXL) return ASRX_ERR_UNSUPPORTED;
  if (tgt_stride < max_target_len) return ASRX_ERR_ARG;
  if (!own_ok || (max_target_len > 0 && !targets)) return ASRX_ERR_ARG;
  if ((int64_t)B * T > 0x7fffffffLL / 4 || B > 65535) return ASRX_ERR_UNSUPPORTED;
  return ASRX_OK;
}

struct ClWs {
  float* stats;   // [B*T][2]: row max, log2 sum
  int* aux;       // [B][CL_AUX]
  float* nll2;    // [B]: -log2 P
  float* alpha;   // [B*T][512*NW]: pair u at [2u] (blank state 2u), [2u + 1] (label state 2u + 1)
  float* beta;
};

inline int64_t cl_r4(int64_t x) { return (x + 3) & ~(int64_t)3; }
inline int64_t cl_ws_elems(int64_t B, int64_t T, int max_l) {
  return cl_r4(2 * B * T) + cl_r4(B * CL_AUX) + cl_r4(B) + 2 * B * T * 512 * cl_nw(max_l);
}
inline ClWs cl_ws(float* ws, int64_t B, int64_t T, int max_l) {
  ClWs w;
  w.stats = ws;
  w.aux = (int*)(ws + cl_r4(2 * B * T));
  w.nll2 = ws + cl_r4(2 * B * T) + cl_r4(B * CL_AUX);
  w.alpha = w.nll2 + cl_r4(B);
  w.beta = w.alpha + B * T * 512 * cl_nw(max_l);
  return w;
}
inline int64_t cl_align_ws_words(int64_t B, int64_t T, int max_l) { return 2 * B * T + 32 * B * T * cl_nw(max_l); }

// ---------------------------------------------------------------------------------------------- loss 1. prep
// blocks [0, B): per sample, validate the target and rank its positions by (label, position), O(L^2) over LDS;
// the other blocks, one wave per (b, t) row: row maximum and log2 sum (ctc_prep_kernel's)
__global__ __launch_bounds__(256) void ctcl_prep_kernel(const float* __restrict__ logits, int B, int T, int V, int64_t ld,
                                                        const int64_t* __restrict__ targets, int64_t tgt_stride,
                                                        const int32_t* __restrict__ input_lengths,
                                                        const int32_t* __restrict__ target_lengths, int max_l,
                                                        int blank, int vec, float* __restrict__ stats,
                                                        int* __restrict__ aux) {
  __shared__ int s_tgt[CL_SLOTS];
  const int tid = threadIdx.x;
  if ((int)blockIdx.x < B) {   // (the whole workgroup takes this branch)
    const int b = blockIdx.x;
    int L = target_lengths[b];
    const bool len_ok = L >= 0 && L <= max_l;
    if (!len_ok) L = 0;
    int bad = 0;
    for (int u = tid; u < L; u += 256) {
      const int64_t id = targets[(int64_t)b * tgt_stride + u];
      const bool bd = id < 0 || id >= V || id == blank;
      bad |= bd;
      s_tgt[u] = bd ? -1 : (int)id;
    }
    bad = __syncthreads_or(bad);
    for (int p = tid; p < max_l; p += 256) {
      int word = 0;
      if (p < L && !bad) {   // (a malformed sample's ranks are never read)
        const int lab = s_tgt[p];
        int less = 0, eq_before = 0, eq_after = 0;
        for (int u = 0; u < L; ++u) {
          const int o = s_tgt[u];
          less += o < lab;
          eq_before += (o == lab) & (u < p);
          eq_after += (o == lab) & (u > p);
        }
        word = (less + eq_before) | ((eq_before == 0 ? 1 + eq_after : 0) << 16);
      }
      aux[(int64_t)b * CL_AUX + p] = word;
    }
    if (tid == 0) {
      const int Tb = clamp_len(input_lengths ? input_lengths[b] : T, T);
      aux[(int64_t)b * CL_AUX + CL_SLOTS] = (len_ok && !bad) ? L : -1;
      aux[(int64_t)b * CL_AUX + CL_SLOTS + 1] = Tb;
    }
    return;
  }
  const int l = tid & 63;
  const int64_t r = ((int64_t)blockIdx.x - B) * 4 + (tid >> 6);
  if (r >= (int64_t)B * T) return;   // (no barrier on this branch)
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

// ---------------------------------------------------------------------------------------------- loss 2. alpha / beta
// grid (B, 2): y = 0 alpha forward in time, y = 1 beta backward; 64 * nw threads
__global__ __launch_bounds__(1024) void ctcl_chain_kernel(const float* __restrict__ logits, int T, int64_t ld,
                                                          const int64_t* __restrict__ targets, int64_t tgt_stride,
                                                          int blank, int nw, ClWs w, float* __restrict__ nll) {
  // per frame parity and wave: [0] lane 63's last label state, [1] lane 0's first blank state, [2] its first label
  __shared__ float s_seam[2][CL_MAXNW][4];
  __shared__ float s_fin[2];
  constexpr int KP = CL_KP;
  const int b = blockIdx.x, dir = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int L = w.aux[(int64_t)b * CL_AUX + CL_SLOTS], Tb = w.aux[(int64_t)b * CL_AUX + CL_SLOTS + 1];
  if (L < 0 || Tb <= 0) {   // no alignment (an empty target over no frames has the empty one); workgroup-uniform
    if (dir == 0 && tid == 0) {
      const float v = (L == 0) ? 0.f : INFINITY;
      nll[b] = v;
      w.nll2[b] = v;
    }
    return;
  }
  // this thread's pairs: label column, validity, and whether the skip transition (s - 2 -> s) exists
  int lab[KP];
  bool vb[KP], vl[KP], skip[KP];
  const int64_t* tg = targets + (int64_t)b * tgt_stride;
#pragma unroll
  for (int q = 0; q < KP; ++q) {
    const int u = tid * KP + q;
    vb[q] = u <= L;
    vl[q] = u < L;
    lab[q] = vl[q] ? (int)tg[u] : blank;
    // alpha: label u from label u - 1; beta: label u from label u + 1 (read from the targets: it may sit in another wave)
    const int o = dir == 0 ? u - 1 : u + 1;
    skip[q] = vl[q] && o >= 0 && o < L && (int)tg[o] != lab[q];
  }
  float sb[KP], sl[KP];   // log2 alpha (beta) of the blank and label state of each pair at the previous step
#pragma unroll
  for (int q = 0; q < KP; ++q) {
    sb[q] = -INFINITY;
    sl[q] = -INFINITY;
    // virtual step before the first: all mass in blank state 0 (alpha) / blank state 2L (beta)
    if (tid * KP + q == (dir == 0 ? 0 : L)) sb[q] = 0.f;
  }
  if (lane == 63) s_seam[0][wv][0] = sl[KP - 1];
  if (lane == 0) {
    s_seam[0][wv][1] = sb[0];
    s_seam[0][wv][2] = sl[0];
  }
  __syncthreads();
  float* out = dir == 0 ? w.alpha : w.beta;
  const int64_t row0 = (int64_t)b * T;
  const int64_t rs = (int64_t)512 * nw;

  float n_b[CL_U], n_l[CL_U][KP], n_m[CL_U], n_s[CL_U];
  auto load = [&](int k0) {
#pragma unroll
    for (int i = 0; i < CL_U; ++i) {
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
  for (int k0 = 0; k0 < Tb; k0 += CL_U) {   // (T_b trips of the frame body, one barrier each, in every wave)
    float c_b[CL_U], c_l[CL_U][KP], c_m[CL_U], c_s[CL_U];
#pragma unroll
    for (int i = 0; i < CL_U; ++i) {
      c_b[i] = n_b[i];
      c_m[i] = n_m[i];
      c_s[i] = n_s[i];
#pragma unroll
      for (int q = 0; q < KP; ++q) c_l[i][q] = n_l[i][q];
    }
    load(k0 + CL_U);
#pragma unroll
    for (int i = 0; i < CL_U; ++i) {
      if (k0 + i >= Tb) break;
      const int par = i & 1;   // = (k0 + i) & 1
      const int64_t r = row0 + (dir == 0 ? k0 + i : Tb - 1 - (k0 + i));
      const float eb = (c_b[i] - c_m[i]) * kLog2e - c_s[i];
      float nb[KP], nl[KP];
      if (dir == 0) {
        const float seam = wv > 0 ? s_seam[par][wv - 1][0] : -INFINITY;
        const float in_l = wave_up1(sl[KP - 1], seam);   // label state of pair u - 1 for q = 0
#pragma unroll
        for (int q = 0; q < KP; ++q) {
          const float pl = q == 0 ? in_l : sl[q - 1];
          const float el = (c_l[i][q] - c_m[i]) * kLog2e - c_s[i];
          nb[q] = vb[q] ? lae2(sb[q], pl) + eb : -INFINITY;
          nl[q] = vl[q] ? lae3(sl[q], sb[q], skip[q] ? pl : -INFINITY) + el : -INFINITY;
        }
      } else {
        const float seam_b = wv + 1 < nw ? s_seam[par][wv + 1][1] : -INFINITY;
        const float seam_l = wv + 1 < nw ? s_seam[par][wv + 1][2] : -INFINITY;
        const float in_b = wave_down1(sb[0], seam_b);      // pair u + 1 for q = KP - 1
        const float in_l = wave_down1(sl[0], seam_l);
#pragma unroll
        for (int q = 0; q < KP; ++q) {
          const float xb = q == KP - 1 ? in_b : sb[q + 1 < KP ? q + 1 : q];
          const float xl = q == KP - 1 ? in_l : sl[q + 1 < KP ? q + 1 : q];
          const float el = (c_l[i][q] - c_m[i]) * kLog2e - c_s[i];
          nb[q] = vb[q] ? lae2(sb[q], sl[q]) + eb : -INFINITY;
          nl[q] = vl[q] ? lae3(sl[q], xb, skip[q] ? xl : -INFINITY) + el : -INFINITY;
        }
      }
      f2_t* o = (f2_t*)(out + r * rs + tid * (2 * KP));
#pragma unroll
      for (int q = 0; q < KP; ++q) {
        sb[q] = nb[q];
        sl[q] = nl[q];
        o[q] = (f2_t){nb[q], nl[q]};
      }
      if (lane == 63) s_seam[par ^ 1][wv][0] = sl[KP - 1];
      if (lane == 0) {
        s_seam[par ^ 1][wv][1] = sb[0];
        s_seam[par ^ 1][wv][2] = sl[0];
      }
      __syncthreads();
    }
  }
  if (dir == 0) {   // P = alpha_T(2L) + alpha_T(2L - 1); (dir is the workgroup's)
#pragma unroll
    for (int q = 0; q < KP; ++q) {
      const int u = tid * KP + q;
      if (u == L) s_fin[0] = sb[q];
      if (L > 0 && u == L - 1) s_fin[1] = sl[q];
    }
    if (tid == 0 && L == 0) s_fin[1] = -INFINITY;
    __syncthreads();
    if (tid == 0) {
      const float p2 = lae2(s_fin[0], s_fin[1]);
      w.nll2[b] = -p2;
      nll[b] = -p2 * kLn2;
    }
  }
}

// ---------------------------------------------------------------------------------------------- loss 3. gradient
template <typename OutT> ASRX_DEV void cl_store4(OutT* p, f4_t g);
template <> ASRX_DEV void cl_store4<float>(float* p, f4_t g) { *(f4_t*)p = g; }
template <> ASRX_DEV void cl_store4<bf16_t>(bf16_t* p, f4_t g) {
  *(v2u_t*)p = (v2u_t){pack2bf(g[0], g[1]), pack2bf(g[2], g[3])};
}
template <typename OutT> ASRX_DEV void cl_store1(OutT* p, float g);
template <> ASRX_DEV void cl_store1<float>(float* p, float g) { *p = g; }
template <> ASRX_DEV void cl_store1<bf16_t>(bf16_t* p, float g) { *p = f2bf(g); }

// one workgroup of 256 threads per (b, t) row.  Dynamic LDS: cl[4096] (label contributions in rank order) then
// occ[ldp] (occupancy per column).  The blank's occupancy: per-thread partial sums over u = tid, tid + 256, .., the
// wave ladder, then the four waves' sums in wave order; a label's: its run of cl, front to back.
template <typename OutT>
__global__ __launch_bounds__(256) void ctcl_grad_kernel(const float* __restrict__ logits, int B, int T, int V, int64_t ld,
                                                        int ldp, const int64_t* __restrict__ targets,
                                                        int64_t tgt_stride, int blank, int nw, int mean,
                                                        int zero_infinity, float grad_scale, int vec, ClWs w,
                                                        OutT* __restrict__ dlogits) {
  extern __shared__ float s_grad[];
  __shared__ float s_part[4];
  float* cl = s_grad;
  float* occ = s_grad + CL_SLOTS;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int64_t r = blockIdx.x;
  const int b = (int)(r / T), t = (int)(r - (int64_t)b * T);
  const int* aux = w.aux + (int64_t)b * CL_AUX;
  const int L = aux[CL_SLOTS], Tb = aux[CL_SLOTS + 1];
  const float nll2 = w.nll2[b];
  const bool feasible = L >= 0 && nll2 < INFINITY;
  const bool live = t < Tb && feasible;   // (the row's: workgroup-uniform)
  const float* x = logits + r * ld;
  const int64_t* tg = targets + (int64_t)b * tgt_stride;
  float mx = 0.f, l2s = 0.f;
  if (live) {
    mx = w.stats[2 * r];
    l2s = w.stats[2 * r + 1];
    for (int c = tid; c < ldp; c += 256) occ[c] = 0.f;
    const float eb = (x[blank] - mx) * kLog2e - l2s;
    float bsum = 0.f;
    const float* al = w.alpha + r * ((int64_t)512 * nw);
    const float* be = w.beta + r * ((int64_t)512 * nw);
    for (int u = tid; u <= L; u += 256) {
      const f2_t a = *(const f2_t*)(al + 2 * u), bt = *(const f2_t*)(be + 2 * u);
      bsum += exp2_raw(a[0] + bt[0] - eb + nll2);
      if (u < L) {
        const int lab = (int)tg[u];   // validated by the prep launch
        const float el = (x[lab] - mx) * kLog2e - l2s;
        cl[aux[u] & 0xffff] = exp2_raw(a[1] + bt[1] - el + nll2);
      }
    }
    bsum = wave_sum(bsum);
    if (lane == 0) s_part[wv] = bsum;
  }
  __syncthreads();
  if (live) {
    if (tid == 0) occ[blank] = ((s_part[0] + s_part[1]) + s_part[2]) + s_part[3];
    for (int u = tid; u < L; u += 256) {
      const int aw = aux[u];
      const int cnt = aw >> 16;
      if (cnt > 0) {   // first occurrence of its label: the label's run, front to back
        const float* run = cl + (aw & 0xffff);
        float s = run[0];
        for (int k = 1; k < cnt; ++k) s += run[k];
        occ[(int)tg[u]] = s;
      }
    }
  }
  __syncthreads();
  OutT* g = dlogits + r * ld;
  const bool nan_row = t < Tb && !feasible && !zero_infinity;
  float gs = grad_scale;
  if (mean) gs = gs / ((float)B * (float)(L > 1 ? L : 1));
  const float dead = nan_row ? __builtin_nanf("") : 0.f;
  if (vec) {
    for (int c0 = tid * 4; c0 < (int)ld; c0 += 1024) {
      f4_t o = {0.f, 0.f, 0.f, 0.f};
      if (c0 < V) {
        const f4_t v = *(const f4_t*)(x + c0);
#pragma unroll
        for (int k = 0; k < 4; ++k)
          if (c0 + k < V) o[k] = live ? gs * (exp2_raw((v[k] - mx) * kLog2e - l2s) - occ[c0 + k]) : dead;
      }
      cl_store4<OutT>(g + c0, o);
    }
  } else {
    for (int c = tid; c < (int)ld; c += 256) {
      float o = 0.f;
      if (c < V) o = live ? gs * (exp2_raw((x[c] - mx) * kLog2e - l2s) - occ[c]) : dead;
      cl_store1<OutT>(g + c, o);
    }
  }
}

// ---------------------------------------------------------------------------------------------- loss 4. loss
__global__ __launch_bounds__(64) void ctcl_finish_kernel(const float* __restrict__ nll, int B,
                                                         const int* __restrict__ aux, int mean, int zero_infinity,
                                                         const float* __restrict__ loss_add, float loss_add_scale,
                                                         float loss_scale, float* __restrict__ loss) {
  const int lane = threadIdx.x;
  float s = 0.f;
  for (int b = lane; b < B; b += 64) {
    float v = nll[b];
    if (zero_infinity && v == INFINITY) v = 0.f;
    if (mean) {
      const int L = aux[(int64_t)b * CL_AUX + CL_SLOTS];
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

// ---------------------------------------------------------------------------------------------- align 1. row logsumexp
__global__ __launch_bounds__(256) void ctcl_rows_lse_kernel(const float* __restrict__ logits, int64_t rows, int V,
                                                            int64_t ld, float* __restrict__ lse) {
  const int l = threadIdx.x & 63;
  const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= rows) return;   // (no barrier in this kernel)
  const float* x = logits + r * ld;
  float mx = -INFINITY, sum = 0.f;
  for (int c = l; c < V; c += 64) mx = fmaxf(mx, x[c]);
  mx = wave_max(mx);
  for (int c = l; c < V; c += 64) sum += expf(x[c] - mx);
  sum = wave_sum(sum);
  if (l == 0) lse[r] = mx + logf(sum);
}

// ---------------------------------------------------------------------------------------------- align 2. alignment
// one workgroup of 64 * nw threads per sample: chain, backtrace (wave 0), outputs — ctc_align_kernel's three phases
__global__ __launch_bounds__(1024) void ctcl_align_kernel(const float* __restrict__ logits, int T, int V, int64_t ld,
                                                          const int64_t* __restrict__ targets, int64_t tgt_stride,
                                                          const int32_t* __restrict__ input_lengths,
                                                          const int32_t* __restrict__ target_lengths, int max_l,
                                                          int blank, int nw, const float* __restrict__ lse_all,
                                                          int32_t* path_all, uint16_t* bp_all, int32_t* frame_pos,
                                                          float* frame_logp, int32_t* tok_start, int32_t* tok_end,
                                                          float* tok_conf, float* score) {
  __shared__ int s_start[CL_SLOTS], s_end[CL_SLOTS];
  __shared__ float s_seam[2][CL_MAXNW];   // per frame parity and wave: lane 63's last label state
  __shared__ float s_wmax[CL_MAXNW];      // per wave: its best state after the last frame of a group of four
  __shared__ int s_rep[CL_MAXNW];
  __shared__ float s_fin[2];
  constexpr int KP = CL_KP;
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, nthr = 64 * nw;
  int L = target_lengths[b];
  const bool len_ok = L >= 0 && L <= max_l;
  if (!len_ok) L = 0;
  const int Tb = clamp_len(input_lengths ? input_lengths[b] : T, T);
  const int64_t* tg = targets + (int64_t)b * tgt_stride;
  const int64_t row0 = (int64_t)b * T;
  const float* lse = lse_all + row0;
  int32_t* path = path_all + row0;
  uint16_t* bp = bp_all + row0 * nthr;

  // this thread's pairs: label column (a bad label is never an index), validity, whether the skip s - 2 -> s exists
  int lab[KP];
  bool vb[KP], vl[KP], skip[KP];
  int bad = 0, rep = 0;
#pragma unroll
  for (int q = 0; q < KP; ++q) {
    const int u = tid * KP + q;
    vb[q] = u <= L;
    vl[q] = u < L;
    const int64_t id = vl[q] ? tg[u] : 0;
    const bool bd = vl[q] && (id < 0 || id >= V || id == blank);
    bad |= bd;
    lab[q] = (vl[q] && !bd) ? (int)id : blank;
    // the previous label from the targets (it may sit in another wave); a bad one there makes the sample infeasible
    const int64_t pid = (vl[q] && u > 0) ? tg[u - 1] : -1;
    const bool same = vl[q] && u > 0 && pid == id;
    skip[q] = vl[q] && u > 0 && !same;
    rep += __popcll(__ballot(same));
  }
  if (lane == 0) s_rep[wv] = rep;
  bad = __syncthreads_or(bad);
  rep = 0;
  for (int i = 0; i < nw; ++i) rep += s_rep[i];
  bool ok = len_ok && !bad && Tb >= L + rep;   // (workgroup-uniform)

  int end = 0;
  float sc = -INFINITY;
  if (ok) {
    float sb[KP], sl[KP];   // best path score into the blank and label state of each pair at the previous frame
    float wm = -INFINITY;
#pragma unroll
    for (int q = 0; q < KP; ++q) {
      sb[q] = -INFINITY;
      sl[q] = -INFINITY;
      if (tid * KP + q == 0) sb[q] = 0.f;   // virtual frame before the first: everything in blank state 0
      wm = fmaxf(wm, sb[q]);
    }
    wm = wave_max_dpp(wm);
    if (lane == 63) s_seam[0][wv] = sl[KP - 1];
    if (lane == 0) s_wmax[wv] = wm;
    __syncthreads();
    double off = 0.0;
    float n_b[CL_U], n_l[CL_U][KP], n_s[CL_U];
    auto load = [&](int k0) {
#pragma unroll
      for (int i = 0; i < CL_U; ++i) {
        int k = k0 + i;
        k = k < Tb ? k : Tb - 1;
        const float* x = logits + (row0 + k) * ld;
        n_b[i] = x[blank];
#pragma unroll
        for (int q = 0; q < KP; ++q) n_l[i][q] = x[lab[q]];
        n_s[i] = lse[k];
      }
    };
    if (Tb > 0) load(0);
    for (int k0 = 0; k0 < Tb; k0 += CL_U) {   // (T_b trips of the frame body, one barrier each, in every wave)
      float c_b[CL_U], c_l[CL_U][KP], c_s[CL_U];
#pragma unroll
      for (int i = 0; i < CL_U; ++i) {
        c_b[i] = n_b[i];
        c_s[i] = n_s[i];
#pragma unroll
        for (int q = 0; q < KP; ++q) c_l[i][q] = n_l[i][q];
      }
      load(k0 + CL_U);
      // renormalise by the workgroup's best state (published before the previous frame's barrier)
      float m = -INFINITY;
      for (int i = 0; i < nw; ++i) m = fmaxf(m, s_wmax[i]);
      if (!(m > -INFINITY) || m == INFINITY) m = 0.f;
      off += (double)m;
#pragma unroll
      for (int q = 0; q < KP; ++q) {
        sb[q] -= m;
        sl[q] -= m;
      }
#pragma unroll
      for (int i = 0; i < CL_U; ++i) {
        if (k0 + i >= Tb) break;
        const int par = i & 1;   // = (k0 + i) & 1
        const float eb = c_b[i] - c_s[i];
        float seam = wv > 0 ? s_seam[par][wv - 1] : -INFINITY;
        if (i == 0) seam -= m;   // (published before this group's renormalisation)
        const float in_l = wave_up1(sl[KP - 1], seam);   // label state of pair u - 1 for q = 0
        float nb[KP], nl[KP];
        unsigned word = 0;
#pragma unroll
        for (int q = 0; q < KP; ++q) {
          const float pl = q == 0 ? in_l : sl[q - 1];
          const float el = c_l[i][q] - c_s[i];
          const bool bfrom = pl > sb[q];
          const float bbest = bfrom ? pl : sb[q];
          float lbest = sl[q];
          unsigned lfrom = 0;
          if (sb[q] > lbest) {
            lbest = sb[q];
            lfrom = 1;
          }
          if (skip[q] && pl > lbest) {
            lbest = pl;
            lfrom = 2;
          }
          nb[q] = vb[q] ? bbest + eb : -INFINITY;
          nl[q] = vl[q] ? lbest + el : -INFINITY;
          word |= ((bfrom ? 1u : 0u) | (lfrom << 1)) << (3 * q);
        }
#pragma unroll
        for (int q = 0; q < KP; ++q) {
          sb[q] = nb[q];
          sl[q] = nl[q];
        }
        bp[(int64_t)(k0 + i) * nthr + tid] = (uint16_t)word;
        if (i == CL_U - 1) {   // the next group's renormaliser
          float v = -INFINITY;
#pragma unroll
          for (int q = 0; q < KP; ++q) v = fmaxf(v, fmaxf(sb[q], sl[q]));
          v = wave_max_dpp(v);
          if (lane == 0) s_wmax[wv] = v;
        }
        if (lane == 63) s_seam[par ^ 1][wv] = sl[KP - 1];
        __syncthreads();
      }
    }
    // the end state: 2L unless the last label state 2L - 1 is at least as good
#pragma unroll
    for (int q = 0; q < KP; ++q) {
      const int u = tid * KP + q;
      if (u == L) s_fin[0] = sb[q];
      if (L > 0 && u == L - 1) s_fin[1] = sl[q];
    }
    if (tid == 0 && L == 0) s_fin[1] = -INFINITY;
    __syncthreads();
    const float fb = s_fin[0], fl = s_fin[1];
    const bool end_blank = L == 0 || fb > fl;
    end = end_blank ? 2 * L : 2 * L - 1;
    sc = (float)(off + (double)(end_blank ? fb : fl));
    ok = sc > -INFINITY;   // (-inf or NaN logits on every path: no alignment)
    if (!ok) sc = -INFINITY;
  }
  for (int i = tid; i < CL_SLOTS; i += nthr) {
    s_start[i] = -1;
    s_end[i] = -1;
  }
  __syncthreads();   // the other waves' backpointers are read below

  // ---- backtrace: a plain dependent walk over the workspace words by wave 0 (lane 0 records the states)
  if (ok && wv == 0) {
    int s = end;
    for (int t = Tb - 1; t >= 0; --t) {
      if (lane == 0) path[t] = s;
      if (t > 0) {
        const int u = s >> 1;
        const unsigned bits = (unsigned)bp[(int64_t)t * nthr + u / KP] >> (3 * (u % KP));
        const int step = (s & 1) ? (int)((bits >> 1) & 3u) : (int)(bits & 1u);
        s -= step;
        s = s < 0 ? 0 : s;
      }
    }
  }
  __syncthreads();

  // ---- per frame: position, log-probability, run boundaries
  for (int t = tid; t < T; t += nthr) {
    int pos = -1;
    float lpv = 0.f;
    if (ok && t < Tb) {
      const int s = path[t];
      const int u = s >> 1;
      int sym = blank;
      if ((s & 1) && u < L) {
        pos = u;
        sym = (int)tg[u];
        if (t == 0 || path[t - 1] != s) s_start[u] = t;
        if (t == Tb - 1 || path[t + 1] != s) s_end[u] = t + 1;
      }
      lpv = logits[(row0 + t) * ld + sym] - lse[t];
    }
    frame_pos[row0 + t] = pos;
    frame_logp[row0 + t] = lpv;
  }
  __syncthreads();

  // ---- per token: span and confidence (the run's log-probabilities again, in frame order)
  for (int u = tid; u < max_l; u += nthr) {
    int st = -1, en = -1;
    float conf = 0.f;
    if (ok && u < L) {
      st = s_start[u];
      en = s_end[u];
      const int c = (int)tg[u];
      float sum = 0.f;
      for (int t = st; t < en; ++t) sum += logits[(row0 + t) * ld + c] - lse[t];
      conf = expf(sum / (float)(en - st));
    }
    tok_start[(int64_t)b * max_l + u] = st;
    tok_end[(int64_t)b * max_l + u] = en;
    tok_conf[(int64_t)b * max_l + u] = conf;
  }
  if (tid == 0) score[b] = sc;
}

}  // namespace

extern "C" int asrx_ctc_long_workspace_elems(int32_t B, int32_t T, int32_t max_target_len, int64_t* elems) {
  const bool ok = B > 0 && T > 0 && max_target_len >= 0 && max_target_len <= CL_MAXL;
  if (elems) *elems = ok ? cl_ws_elems(B, T, max_target_len) : -1;
  return ok && elems ? ASRX_OK : ASRX_ERR_ARG;
}

extern "C" int asrx_ctc_loss_long(const float* logits, int32_t B, int32_t T, int32_t V, int64_t ld,
                                  const int64_t* targets, int64_t tgt_stride, const int32_t* input_lengths,
                                  const int32_t* target_lengths, int32_t max_target_len, int32_t blank,
                                  int32_t reduction, int32_t zero_infinity, float grad_scale, float* nll, float* loss,
                                  void* dlogits, int32_t dlogits_dtype, const float* loss_add, float loss_add_scale,
                                  float loss_scale, float* ws, int64_t ws_elems, void* stream) {
  if (reduction != ASRX_CTC_SUM && reduction != ASRX_CTC_MEAN) return ASRX_ERR_ARG;
  if (dlogits && dlogits_dtype != ASRX_BF16 && dlogits_dtype != ASRX_F32) return ASRX_ERR_ARG;
  const bool own_ok = logits && target_lengths && nll && loss && ws && ((uintptr_t)ws & 15) == 0 &&
                      ws_elems >= cl_ws_elems(B, T, std::min(std::max(max_target_len, 0), CL_MAXL));
  const int err = cl_check_target_args(B, T, V, ld, targets, tgt_stride, max_target_len, blank, own_ok);
  if (err != ASRX_OK) return err;
  if (ld > 8192) return ASRX_ERR_UNSUPPORTED;   // the gradient's occupancy row lives in LDS
  hipStream_t st = (hipStream_t)stream;
  const ClWs w = cl_ws(ws, B, T, max_target_len);
  const int nw = cl_nw(max_target_len);
  const int64_t rows = (int64_t)B * T;
  const int mean = reduction == ASRX_CTC_MEAN;
  const int vec_in = ld % 4 == 0 && ((uintptr_t)logits & 15) == 0;
  const int64_t* tg = ctc_targets_or_dummy(targets);

  hipLaunchKernelGGL(ctcl_prep_kernel, dim3((unsigned)(B + (rows + 3) / 4)), dim3(256), 0, st, logits, B, T, V, ld, tg,
                     tgt_stride, input_lengths, target_lengths, max_target_len, blank, vec_in, w.stats, w.aux);
  ASRX_CHECK_LAUNCH();
  hipLaunchKernelGGL(ctcl_chain_kernel, dim3((unsigned)B, 2), dim3(64 * nw), 0, st, logits, T, ld, tg, tgt_stride,
                     blank, nw, w, nll);
  ASRX_CHECK_LAUNCH();
  if (dlogits) {
    const int ldp = (int)((ld + 3) & ~(int64_t)3);
    const size_t shm = sizeof(float) * (CL_SLOTS + ldp);
    if (dlogits_dtype == ASRX_F32) {
      const int vec = vec_in && ((uintptr_t)dlogits & 15) == 0;
      hipLaunchKernelGGL(ctcl_grad_kernel<float>, dim3((unsigned)rows), dim3(256), shm, st, logits, B, T, V, ld, ldp,
                         tg, tgt_stride, blank, nw, mean, zero_infinity, grad_scale, vec, w, (float*)dlogits);
    } else {
      const int vec = vec_in && ((uintptr_t)dlogits & 7) == 0;
      hipLaunchKernelGGL(ctcl_grad_kernel<bf16_t>, dim3((unsigned)rows), dim3(256), shm, st, logits, B, T, V, ld, ldp,
                         tg, tgt_stride, blank, nw, mean, zero_infinity, grad_scale, vec, w, (bf16_t*)dlogits);
    }
    ASRX_CHECK_LAUNCH();
  }
  hipLaunchKernelGGL(ctcl_finish_kernel, dim3(1), dim3(64), 0, st, nll, B, w.aux, mean, zero_infinity, loss_add,
                     loss_add_scale, loss_scale, loss);
  ASRX_CHECK_LAUNCH();
  return ASRX_OK;
}

extern "C" int asrx_ctc_align_long_workspace_words(int32_t B, int32_t T, int32_t max_target_len, int64_t* words) {
  const bool ok = B > 0 && T > 0 && max_target_len >= 0 && max_target_len <= CL_MAXL;
  if (words) *words = ok ? cl_align_ws_words(B, T, max_target_len) : -1;
  return ok && words ? ASRX_OK : ASRX_ERR_ARG;
}

extern "C" int asrx_ctc_align_long(const float* logits, int32_t B, int32_t T, int32_t V, int64_t ld,
                                   const int64_t* targets, int64_t tgt_stride, const int32_t* input_lengths,
                                   const int32_t* target_lengths, int32_t max_target_len, int32_t blank, void* ws,
                                   int64_t ws_words, int32_t* frame_pos, float* frame_logp, int32_t* tok_start,
                                   int32_t* tok_end, float* tok_conf, float* score, void* stream) {
  const bool own_ok = logits && target_lengths && ws && frame_pos && frame_logp && score &&
                      (max_target_len <= 0 || (tok_start && tok_end && tok_conf)) && ((uintptr_t)ws & 3) == 0 &&
                      ws_words >= cl_align_ws_words(B, T, std::min(std::max(max_target_len, 0), CL_MAXL));
  const int err = cl_check_target_args(B, T, V, ld, targets, tgt_stride, max_target_len, blank, own_ok);
  if (err != ASRX_OK) return err;
  hipStream_t st = (hipStream_t)stream;
  const int nw = cl_nw(max_target_len);
  const int64_t rows = (int64_t)B * T;
  float* lse = (float*)ws;
  int32_t* path = (int32_t*)ws + rows;
  uint16_t* bp = (uint16_t*)((int32_t*)ws + 2 * rows);
  const int64_t* tg = ctc_targets_or_dummy(targets);

  hipLaunchKernelGGL(ctcl_rows_lse_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, st, logits, rows, (int)V, ld,
                     lse);
  ASRX_CHECK_LAUNCH();
  hipLaunchKernelGGL(ctcl_align_kernel, dim3((unsigned)B), dim3(64 * nw), 0, st, logits, (int)T, (int)V, ld, tg,
                     tgt_stride, input_lengths, target_lengths, (int)max_target_len, (int)blank, nw, (const float*)lse,
                     path, bp, frame_pos, frame_logp, tok_start, tok_end, tok_conf, score);
  ASRX_CHECK_LAUNCH();
  return ASRX_OK;
}
