// CTC forced alignment: the best (Viterbi) CTC path through the encoder frames that collapses to a given transcript,
// and from it per-frame target positions, per-token frame spans and confidences.  C-ABI: asrx_ctc_align,
// asrx_ctc_align_workspace_words (include/asrx.h).
//
// Two launches on one stream, natural-log domain:
//   1. align_rows_kernel   one wave per (b, t) row: logsumexp of the row -> ws (lp[t][c] = logits[t][c] - lse[t]).
//   2. ctc_align_kernel    one wave64 per sample, three phases.
//      chain      asrx_ctc_loss's alpha recursion with max in place of log-sum-exp: the sample's 2L + 1 extended
//                 states are L + 1 (blank, label) PAIRS, lane i owning pairs i*KP .. i*KP + KP - 1 in registers
//                 (KP = ceil((Lmax + 1) / 64) <= 4, hence L <= 255); the one value a pair needs from lane i - 1 comes
//                 by a DPP wave shift, the emissions of the next four frames are loaded while the current four are
//                 computed, and the loop has no barrier.  Every four frames the states are renormalised by the best
//                 one (decisions depend on differences only), the offsets summed in a double and added back into
//                 the score.  A frame's backpointers are 3 bits per pair: bit 0, the blank state came from the
//                 previous pair's label (else stayed); bits 1-2, the label state stayed (0), came from its own
//                 blank (1) or skipped from the previous label (2).  That is one 16-bit word per lane and frame,
//                 [frame][lane].  Ties: skip only if strictly greater than both others, else the blank only if
//                 strictly greater than the stay; at the end the final blank only if strictly greater than the last
//                 label.
//      backtrace  frames T_b - 1 .. 1, one backpointer word per frame; the state of every frame -> ws.
//      outputs    frame-parallel: position and log-probability of each frame, the run boundaries through LDS;
//                 token-parallel: spans and exp(mean log-probability of the run), summed in frame order.
// The backpointers live in LDS while T <= 1008 (128 B per frame, with the 2 KiB of run boundaries exactly 128 KiB);
// a longer T keeps them in the workspace instead (asrx_ctc_align_workspace_words grows accordingly).
// No atomics, fixed orders: the same inputs give the same bits.  Every output element is written by every call.
#include "ctc_common.h"

namespace {

constexpr int AL_U = 4;               // frames of emissions in flight (8 measured the same)
constexpr int AL_LDS_T = 1008;        // longest T whose backpointers stay in LDS: 1008 * 128 B + 2 KiB = 128 KiB
constexpr int AL_STATIC_LDS = 2048;   // s_start + s_end

inline int64_t al_ws_words(int64_t B, int64_t T) { return 2 * B * T + (T > AL_LDS_T ? 32 * B * T : 0); }

// ---------------------------------------------------------------------------------------------- 1. row logsumexp
__global__ __launch_bounds__(256) void align_rows_kernel(const float* __restrict__ logits, int64_t rows, int V,
                                                         int64_t ld, float* __restrict__ lse) {
  const int l = threadIdx.x & 63;
  const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= rows) return;
  const float* x = logits + r * ld;
  float mx = -INFINITY, sum = 0.f;
  for (int c = l; c < V; c += 64) mx = fmaxf(mx, x[c]);
  mx = wave_max(mx);
  for (int c = l; c < V; c += 64) sum += expf(x[c] - mx);
  sum = wave_sum(sum);
  if (l == 0) lse[r] = mx + logf(sum);
}

// ---------------------------------------------------------------------------------------------- 2. alignment
// SPILL: the backpointers are in the workspace (bp_all), else in dynamic LDS (T * 128 B)
template <int KP, bool SPILL>
__global__ __launch_bounds__(64) void ctc_align_kernel(const float* __restrict__ logits, int T, int V, int64_t ld,
                                                       const int64_t* __restrict__ targets, int64_t tgt_stride,
                                                       const int32_t* __restrict__ input_lengths,
                                                       const int32_t* __restrict__ target_lengths, int max_l,
                                                       int blank, const float* __restrict__ lse_all,
                                                       int32_t* path_all, uint16_t* bp_all, int32_t* frame_pos,
                                                       float* frame_logp, int32_t* tok_start, int32_t* tok_end,
                                                       float* tok_conf, float* score) {
  __shared__ int s_start[256], s_end[256];
  extern __shared__ uint16_t s_bp[];
  const int b = blockIdx.x, lane = threadIdx.x;
  int L = target_lengths[b];
  const bool len_ok = L >= 0 && L <= max_l;
  if (!len_ok) L = 0;
  const int Tb = clamp_len(input_lengths ? input_lengths[b] : T, T);
  const int64_t* tg = targets + (int64_t)b * tgt_stride;
  const int64_t row0 = (int64_t)b * T;
  const float* lse = lse_all + row0;
  int32_t* path = path_all + row0;
  uint16_t* bp = SPILL ? bp_all + row0 * 64 : s_bp;

  // this lane's pairs: label column (a bad label is never an index), validity, whether the skip s - 2 -> s exists
  int lab[KP];
  bool vb[KP], vl[KP], skip[KP];
  bool bad = false;
  int rep = 0;
#pragma unroll
  for (int q = 0; q < KP; ++q) {
    const int u = lane * KP + q;
    vb[q] = u <= L;
    vl[q] = u < L;
    const int64_t id = vl[q] ? tg[u] : 0;
    const bool bd = vl[q] && (id < 0 || id >= V || id == blank);
    bad |= bd;
    lab[q] = (vl[q] && !bd) ? (int)id : blank;
  }
  const int in_lab = wave_up1(lab[KP - 1], -1);
#pragma unroll
  for (int q = 0; q < KP; ++q) {
    const int u = lane * KP + q;
    const int pl = q == 0 ? in_lab : lab[q - 1];
    skip[q] = vl[q] && u > 0 && pl != lab[q];
    rep += __popcll(__ballot(vl[q] && u > 0 && pl == lab[q]));
  }
  bool ok = len_ok && __ballot(bad) == 0 && Tb >= L + rep;   // (wave-uniform)

  int end = 0;
  float sc = -INFINITY;
  if (ok) {
    float sb[KP], sl[KP];   // best path score into the blank and label state of each pair at the previous frame
#pragma unroll
    for (int q = 0; q < KP; ++q) {
      sb[q] = -INFINITY;
      sl[q] = -INFINITY;
      if (lane * KP + q == 0) sb[q] = 0.f;   // virtual frame before the first: everything in blank state 0
    }
    double off = 0.0;
    float n_b[AL_U], n_l[AL_U][KP], n_s[AL_U];
    auto load = [&](int k0) {
#pragma unroll
      for (int i = 0; i < AL_U; ++i) {
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
    for (int k0 = 0; k0 < Tb; k0 += AL_U) {
      float c_b[AL_U], c_l[AL_U][KP], c_s[AL_U];
#pragma unroll
      for (int i = 0; i < AL_U; ++i) {
        c_b[i] = n_b[i];
        c_s[i] = n_s[i];
#pragma unroll
        for (int q = 0; q < KP; ++q) c_l[i][q] = n_l[i][q];
      }
      load(k0 + AL_U);
      // renormalise by the best state: the compared values stay small whatever T is
      float m = -INFINITY;
#pragma unroll
      for (int q = 0; q < KP; ++q) m = fmaxf(m, fmaxf(sb[q], sl[q]));
      m = wave_max_dpp(m);
      if (!(m > -INFINITY) || m == INFINITY) m = 0.f;
      off += (double)m;
#pragma unroll
      for (int q = 0; q < KP; ++q) {
        sb[q] -= m;
        sl[q] -= m;
      }
#pragma unroll
      for (int i = 0; i < AL_U; ++i) {
        if (k0 + i >= Tb) break;
        const float eb = c_b[i] - c_s[i];
        const float in_l = wave_up1(sl[KP - 1], -INFINITY);   // label state of pair u - 1 for q = 0
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
        bp[(int64_t)(k0 + i) * 64 + lane] = (uint16_t)word;
      }
    }
    // the end state: 2L unless the last label state 2L - 1 is at least as good
    float fb = -INFINITY, fl = -INFINITY;
#pragma unroll
    for (int q = 0; q < KP; ++q) {
      if (q == L % KP) fb = sb[q];
      if (L > 0 && q == (L - 1) % KP) fl = sl[q];
    }
    fb = __shfl(fb, L / KP, 64);
    fl = __shfl(fl, L > 0 ? (L - 1) / KP : 0, 64);
    const bool end_blank = L == 0 || fb > fl;
    end = end_blank ? 2 * L : 2 * L - 1;
    sc = (float)(off + (double)(end_blank ? fb : fl));
    ok = sc > -INFINITY;   // (-inf or NaN logits on every path: no alignment)
    if (!ok) sc = -INFINITY;
  }
  for (int i = lane; i < 256; i += 64) {
    s_start[i] = -1;
    s_end[i] = -1;
  }
  __syncthreads();   // the other lanes' backpointers are read below

  // ---- backtrace (every lane walks the same states; lane 0 records them).  One dependent LDS read per frame; a walk
  // on the scalar unit, each lane reading its own words ahead and the walk picking the owner's by v_readlane, measured
  // 8 us slower at T 249.
  if (ok) {
    int s = end;
    for (int t = Tb - 1; t >= 0; --t) {
      if (lane == 0) path[t] = s;
      if (t > 0) {
        const int u = s >> 1;
        const unsigned bits = (unsigned)bp[(int64_t)t * 64 + u / KP] >> (3 * (u % KP));
        const int step = (s & 1) ? (int)((bits >> 1) & 3u) : (int)(bits & 1u);
        s -= step;
        s = s < 0 ? 0 : s;
      }
    }
  }
  __syncthreads();

  // ---- per frame: position, log-probability, run boundaries
  for (int t = lane; t < T; t += 64) {
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
  for (int u = lane; u < max_l; u += 64) {
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
  if (lane == 0) score[b] = sc;
}

}  // namespace

extern "C" int64_t asrx_ctc_align_workspace_words(int32_t B, int32_t T, int32_t max_target_len) {
  if (B <= 0 || T <= 0 || max_target_len < 0 || max_target_len > CTC_MAXL) return -1;
  return al_ws_words(B, T);
}

extern "C" int asrx_ctc_align(const float* logits, int32_t B, int32_t T, int32_t V, int64_t ld, const int64_t* targets,
                              int64_t tgt_stride, const int32_t* input_lengths, const int32_t* target_lengths,
                              int32_t max_target_len, int32_t blank, void* ws, int64_t ws_words, int32_t* frame_pos,
                              float* frame_logp, int32_t* tok_start, int32_t* tok_end, float* tok_conf, float* score,
                              void* stream) {
  const bool own_ok = logits && target_lengths && ws && frame_pos && frame_logp && score &&
                      (max_target_len <= 0 || (tok_start && tok_end && tok_conf)) && ((uintptr_t)ws & 3) == 0 &&
                      ws_words >= al_ws_words(B, T);
  const int err = ctc_check_target_args(B, T, V, ld, targets, tgt_stride, max_target_len, blank, own_ok);
  if (err != ASRX_OK) return err;
  const bool spill = T > AL_LDS_T;
  const size_t shm = spill ? 0 : (size_t)T * 128;
  if (shm + AL_STATIC_LDS > 128 * 1024) return ASRX_ERR_UNSUPPORTED;   // (cannot happen: AL_LDS_T is that bound)
  hipStream_t st = (hipStream_t)stream;
  const int64_t rows = (int64_t)B * T;
  float* lse = (float*)ws;
  int32_t* path = (int32_t*)ws + rows;
  uint16_t* bp = (uint16_t*)((int32_t*)ws + 2 * rows);   // (spill only: the workspace ends here otherwise)
  const int64_t* tg = ctc_targets_or_dummy(targets);

  hipLaunchKernelGGL(align_rows_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, st, logits, rows, (int)V, ld,
                     lse);
  ASRX_CHECK_LAUNCH();
  ctc_dispatch_kp(ctc_kp(max_target_len), [&](auto kpc) {
    constexpr int KP = decltype(kpc)::value;
    const auto kernel = spill ? ctc_align_kernel<KP, true> : ctc_align_kernel<KP, false>;   // (spill: shm = 0)
    hipLaunchKernelGGL(kernel, dim3((unsigned)B), dim3(64), shm, st, logits, (int)T, (int)V, ld, tg, tgt_stride,
                       input_lengths, target_lengths, (int)max_target_len, (int)blank, (const float*)lse, path, bp,
                       frame_pos, frame_logp, tok_start, tok_end, tok_conf, score);
  });
  ASRX_CHECK_LAUNCH();
  return ASRX_OK;
}
