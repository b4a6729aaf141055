// Two-pass decoding (attention rescoring): the first pass, CTC prefix beam search over the encoder frames without the
// decoder, and the small kernels of the second.  C-ABI: asrx_ctc_prefix_beam, asrx_hyp_tokens, asrx_seq_logprob,
// asrx_rescore_rank (include/asrx.h).
//
// asrx_ctc_prefix_beam: one workgroup per utterance, the frame loop inside the kernel.  A beam slot holds a prefix g
// (its hash h, its parent's hash ph, its last label, a trie node for the backtrack) with (pb, pnb) = the
// log-probability of the paths over the frames so far that collapse to g and end in the blank / in a non-blank,
// tot = logaddexp(pb, pnb).  At frame t, with
// y = log_softmax(logits[t]), the candidates of slot w are
//   column blank   the stay: pb' = tot(w) + y(blank), pnb' = pnb(w) + y(last(w)), to which the one parent of g that
//                  may be in the beam (h(w0) == ph(w)) adds its extension by last(w), stay term first;
//   column c       the extension g.c: pnb' = (c == last(w) ? pb(w) : tot(w)) + y(c); -inf once g has max_labels
//                  labels or where g.c is itself in the beam (its mass went to that slot's stay),
// and the W best by logaddexp(pb', pnb') under asrx_beam_step's total order (score descending, flat index w*V + c
// ascending, NaN read as -inf, -inf never selected) are the next beam, in that order.
//
// What keeps the serial loop short:
//   * A row-parallel prologue (one wave per frame) leaves in the workspace every frame's logsumexp and its 2W largest
//     non-blank logits in the order (value descending, column ascending); up to V = 512 by one counting pass per row
//     (each column counts the columns ranked before it), beyond that by 2W rounds of a wave-wide arg-max.
//   * The loop forms only the candidates that can be selected.  The slots are in score order, so tot(w) does not
//     increase with w, and x -> tot + (x - lse) is monotone: the extension of slot w by the k-th column of the list
//     is preceded by every extension (w' <= w, k' <= k) of a slot that may still extend, except the "special" ones:
//     the column last(w') of each such slot (lower: pb <= tot) and the at most W - 1 columns whose prefix is in the
//     beam (-inf).  With u(w) the number of slots w' <= w below max_labels, at least u*(k + 1) - 1 - u - (W - 1)
//     candidates precede it, so it can be among the W best only if k < 2W / u(w): slot w offers ceil(2W / u(w))
//     list columns, 114 candidates at W = 16 where the full matrix has W * V, plus the W stays.  (Two DIFFERENT
//     logits of a frame whose candidates round to one fp32 value keep the list's order; equal logits are in column
//     order, as the flat index asks.)
//   * Only the W stay candidates take transcendentals; an extension is one add.
//   * The selection is one pass: every candidate counts those ranked before it and, if fewer than W, is the slot of
//     that rank.  Three barriers per frame, all reached by the whole workgroup (the frame count is uniform), and no
//     wait for global memory: the next frame's operands are fetched a frame ahead.
//   * Each frame's scores are renormalised by the frame's best tot; the running offset is a double kept by thread 0,
//     so scores near -900 at T' 249 do not cost the selection its fp32 resolution.
// A fresh extension selected into slot j at frame t is trie node 1 + t*W + j (root 0); its (parent node, token) goes to
// the workspace and the final phase of the same launch walks it back.  fp32, natural log, every log-add
// max-subtracted, no atomics, fixed orders: the same inputs give the same bits.
#include <limits.h>

#include "ctc_common.h"

namespace {

constexpr int CB_THREADS = 512;
constexpr int CB_WAVES = CB_THREADS / 64;
constexpr int CB_MAXW = 16;
constexpr int CB_MAXC = 136;   // sum over w < 16 of ceil(32 / (w + 1)) = 114 extensions, 16 stays, rounded up to 8
constexpr int CB_XR = 8;       // most logits of a row a lane keeps in registers (V <= 512)
constexpr int CB_MAXV = 1 << 20;

// log(e^a + e^b), max-subtracted, on the raw v_exp_f32 / v_log_f32 (absolute error ~1e-7: the argument of the
// logarithm lies in [1, 2]); -inf operands are legal
ASRX_DEV float cb_lae(float a, float b) {
  const float hi = fmaxf(a, b), lo = fminf(a, b);
  if (!(hi > -INFINITY)) return -INFINITY;
  return hi + kLn2 * log2_raw(1.f + exp2_raw((lo - hi) * kLog2e));
}

// A candidate as one 64-bit key: a ranks before b exactly when key(a) > key(b).  High word: the score's bits made
// monotone (-0 folded into +0 first), low word: ~flat index.
typedef uint64_t cb_key2_t __attribute__((ext_vector_type(2)));
ASRX_DEV uint64_t cb_key(float s, int idx) {
  uint32_t u = __float_as_uint(s + 0.f);
  u ^= (u >> 31) ? 0xFFFFFFFFu : 0x80000000u;
  return ((uint64_t)u << 32) | (uint32_t)~idx;
}
ASRX_DEV float cb_key_score(uint64_t k) {
  uint32_t u = (uint32_t)(k >> 32);
  u ^= (u >> 31) ? 0x80000000u : 0xFFFFFFFFu;
  return __uint_as_float(u);
}
ASRX_DEV int cb_key_idx(uint64_t k) { return (int)~(uint32_t)k; }

// Prefix identity.  A trie node id cannot serve: a prefix that is pruned while one of its children stays in the beam
// and is later selected again would come back under a fresh id that the child does not point to.  A slot therefore
// carries a 64-bit hash of its label string, h(g.c) = mix(h(g), c), and its parent's: g.c is slot w' exactly when
// ph(w') == h(w) and last(w') == c, whatever became of the slots in between.  (Two different strings of one beam
// share a hash with probability about 2^-64 per compared pair; the root's parent hash 0 is no slot's hash in the
// same sense.)
constexpr uint64_t CB_ROOT_HASH = 0x243F6A8885A308D3ull;
ASRX_DEV uint64_t cb_hash(uint64_t h, int c) {
  uint64_t z = (h ^ (uint64_t)(uint32_t)(c + 1)) * 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// 4-byte words of workspace per sample: lse [T], top values [T][2W], top columns [T][2W], trie [T*W][2]
ASRX_DEV int64_t cb_ws_words(int T, int W) { return (int64_t)T * (1 + 6 * W); }

// list columns slot w offers when u slots up to and including it may still extend
ASRX_DEV int cb_offer(int W, int u) { return (2 * W + u - 1) / u; }

// XR > 0: a lane keeps XR logits of the row in registers (V <= 64 * XR; 4 or CB_XR); XR = 0: any V, every round of the
// prologue reads the row again (L1 / L2)
template <int XR>
__global__ __launch_bounds__(CB_THREADS) void ctc_prefix_beam_kernel(
    const float* __restrict__ logits, int T, int V, int64_t ld, const int32_t* __restrict__ input_lengths, int blank,
    int W, int max_labels, float* ws, int64_t* __restrict__ tok, int32_t* __restrict__ len,
    float* __restrict__ score, int32_t* __restrict__ n_hyp) {
  __shared__ float s_pb[CB_MAXW], s_pnb[CB_MAXW], s_tot[CB_MAXW], s_spb[CB_MAXW], s_spnb[CB_MAXW];
  __shared__ int s_node[CB_MAXW], s_last[CB_MAXW], s_len[CB_MAXW], s_sel[CB_MAXW];
  __shared__ uint64_t s_h[CB_MAXW], s_ph[CB_MAXW];   // identity of the slot's prefix and of its parent prefix
  __shared__ int s_koff[CB_MAXW];   // the first candidate of slot w's extensions (a slot at max_labels has none)
  __shared__ int s_offer[CB_MAXW];  // list columns the u-th slot that may extend offers, u = 1..W (no division in the loop)
  __shared__ int s_cw[CB_MAXC];     // the slot an extension candidate extends
  __shared__ __attribute__((aligned(16))) uint64_t s_c[CB_MAXC];   // candidate keys: extensions, then the n stays
  __shared__ float s_tx[2 * CB_MAXW], s_lse;   // the frame's list values, its logsumexp
  __shared__ int s_ti[2 * CB_MAXW];            // ... and list columns
  __shared__ int s_n, s_next;
  __shared__ __attribute__((aligned(16))) uint64_t s_row[XR > 0 ? CB_WAVES : 1][64 * (XR > 0 ? XR : 1)];   // the prologue's rows
  __shared__ double s_off;

  constexpr bool REG = XR > 0;
  constexpr int XRC = REG ? XR : 1;
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int K = 2 * W;
  const int Tb = clamp_len(input_lengths ? input_lengths[b] : T, T);
  const float* x0 = logits + (int64_t)b * T * ld;
  float* w_lse = ws + (int64_t)b * cb_ws_words(T, W);
  float* w_topx = w_lse + T;
  int32_t* w_topi = (int32_t*)(w_topx + (int64_t)T * K);
  int32_t* w_trie = w_topi + (int64_t)T * K;

  // ---- prologue: per frame the logsumexp and the K largest non-blank logits in order.  REG: every column counts the
  // columns ranked before it (the row's keys go through this wave's LDS row, read back as broadcasts) and, if fewer
  // than K, is the list entry of that rank: one pass whatever K is.  Else K rounds of a wave-wide arg-max.
  for (int t = wave; t < Tb; t += CB_WAVES) {
    const float* x = x0 + (int64_t)t * ld;
    float xv[XRC];
    float mx = -INFINITY;
    if (REG) {
#pragma unroll
      for (int j = 0; j < XRC; ++j) {
        const int c = lane + 64 * j;
        xv[j] = c < V ? x[c] : -INFINITY;
        mx = fmaxf(mx, xv[j]);
      }
    } else {
      for (int c = lane; c < V; c += 64) mx = fmaxf(mx, x[c]);
    }
    mx = wave_max(mx);
    float sum = 0.f;   // (a NaN logit makes the whole row's lse NaN)
    if (REG) {
#pragma unroll
      for (int j = 0; j < XRC; ++j)
        if (lane + 64 * j < V) sum += expf(xv[j] - mx);
    } else {
      for (int c = lane; c < V; c += 64) sum += expf(x[c] - mx);
    }
    sum = wave_sum(sum);
    if (lane == 0) w_lse[t] = mx + logf(sum);
    if (REG) {
      uint64_t* row = s_row[wave];
      uint64_t key[XRC];   // (0: no column; the key of a real one is never 0)
      int r[XRC];
#pragma unroll
      for (int j = 0; j < XRC; ++j) {
        const int c = lane + 64 * j;
        key[j] = c < V && c != blank ? cb_key(nonan(xv[j]), c) : 0;
        row[c] = key[j];
        r[j] = 0;
      }
      wave_lds_sync();   // the other lanes' keys, written above, are read below
      const cb_key2_t* row2 = (const cb_key2_t*)row;
      const int pairs = (V + 63) / 64 * 32;   // whole 64-column groups: the tail holds zeros
#pragma unroll 4
      for (int i = 0; i < pairs; ++i) {
        const cb_key2_t o = row2[i];
#pragma unroll
        for (int j = 0; j < XRC; ++j) r[j] += (o[0] > key[j] ? 1 : 0) + (o[1] > key[j] ? 1 : 0);
      }
#pragma unroll
      for (int j = 0; j < XRC; ++j) {
        if (key[j] != 0 && r[j] < K) {
          w_topx[(int64_t)t * K + r[j]] = cb_key_score(key[j]);
          w_topi[(int64_t)t * K + r[j]] = lane + 64 * j;
        }
      }
      for (int k = V - 1 + lane; k < K; k += 64) {   // fewer than K non-blank columns: no column
        w_topx[(int64_t)t * K + k] = -INFINITY;
        w_topi[(int64_t)t * K + k] = -1;
      }
    } else {
      float ps = INFINITY;   // the previous pick: round k takes the best column strictly after it
      int pi = -1;
      for (int k = 0; k < K; ++k) {
        float bs = -INFINITY;
        int bi = INT_MAX;
        for (int c = lane; c < V; c += 64) {
          if (c == blank) continue;
          const float v = nonan(x[c]);
          if (ranks_before(ps, pi, v, c) && ranks_before(v, c, bs, bi)) { bs = v; bi = c; }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
          const float os = __shfl_xor(bs, o, 64);
          const int oi = __shfl_xor(bi, o, 64);
          if (ranks_before(os, oi, bs, bi)) { bs = os; bi = oi; }
        }
        if (lane == 0) {
          w_topx[(int64_t)t * K + k] = bs;
          w_topi[(int64_t)t * K + k] = bi == INT_MAX ? -1 : bi;   // (-1: fewer than K non-blank columns)
        }
        ps = bs;
        pi = bi;
      }
    }
  }
  if (tid < CB_MAXW) {   // the root in slot 0
    s_pb[tid] = tid == 0 ? 0.f : -INFINITY;
    s_pnb[tid] = -INFINITY;
    s_tot[tid] = tid == 0 ? 0.f : -INFINITY;
    s_node[tid] = tid == 0 ? 0 : -2;
    s_h[tid] = CB_ROOT_HASH;
    s_ph[tid] = 0;
    s_last[tid] = -1;
    s_len[tid] = 0;
    s_sel[tid] = -1;
    s_koff[tid] = tid == 0 ? 0 : K;
    const int kw = cb_offer(W, tid + 1);
    s_offer[tid] = kw < K ? kw : K;
  }
  if (tid == 0) {
    s_n = 1;
    s_next = K;
  }
  __syncthreads();

  // ---- the frame loop.  Nothing in it waits for global memory: a frame's list, logsumexp and the logits the stays
  // need (the blank's, and each slot's last label's once the slot is known) are fetched one frame ahead, the list
  // through LDS, the stays' operands in the registers of the thread that owns the slot.
  const int lt = tid - 64;   // wave 1..: extension candidate / list entry of this thread
  float xb = 0.f, xl = 0.f;  // tid < W: logits[t][blank], logits[t][last(tid)]
  if (Tb > 0) {
    if (lt >= 0 && lt < K) {
      s_tx[lt] = w_topx[lt];
      s_ti[lt] = w_topi[lt];
    }
    if (tid == 0) s_lse = w_lse[0];
    if (tid < W) xb = x0[blank];
  }
  __syncthreads();
  double off = 0.0;   // thread 0: the sum of the frames' renormalisations
  for (int t = 0; t < Tb; ++t) {
    const int n = s_n;
    if (n == 0) break;   // (uniform: every thread read the same word after a barrier)
    const int next = s_next, nc = next + n, ncp = (nc + 7) & ~7;
    const float lse = s_lse;
    const bool more = t + 1 < Tb;
    const float* xn = x0 + (int64_t)(t + 1) * ld;   // (read only if `more`)
    float p_x = 0.f, p_lse = 0.f, p_xb = 0.f, p_xl = 0.f;
    int p_i = -1;
    if (more) {
      if (lt >= 0 && lt < K) {
        p_x = w_topx[(int64_t)(t + 1) * K + lt];
        p_i = w_topi[(int64_t)(t + 1) * K + lt];
      }
      if (tid < W) p_xb = xn[blank];
      if (tid == 0) p_lse = w_lse[t + 1];
    }
    if (tid < n) {   // the stay of slot tid
      const int w = tid, last = s_last[w];
      const uint64_t ph = s_ph[w];
      float pb = s_tot[w] + (xb - lse);
      float pnb = -INFINITY;
      if (last >= 0) {
        const float yl = xl - lse;
        pnb = s_pnb[w] + yl;
        int w0 = -1;   // the one slot that may hold g's parent
        for (int j = 0; j < n; ++j) w0 = s_h[j] == ph ? j : w0;
        if (w0 >= 0) pnb = cb_lae(pnb, (last == s_last[w0] ? s_pb[w0] : s_tot[w0]) + yl);
      }
      pb = nonan(pb);
      pnb = nonan(pnb);
      s_spb[w] = pb;
      s_spnb[w] = pnb;
      s_c[next + w] = cb_key(cb_lae(pb, pnb), w * V + blank);
    } else if (lt >= 0 && lt < next) {   // an extension
      int w = 0;
      for (int j = 1; j < n; ++j) w += lt >= s_koff[j] ? 1 : 0;
      const int k = lt - s_koff[w];
      const int c = s_ti[k];
      float sc = -INFINITY;
      int idx = INT_MAX;
      if (c >= 0) {
        idx = w * V + c;
        const uint64_t h = s_h[w];
        bool merged = false;
        for (int w1 = 0; w1 < n; ++w1) merged |= s_ph[w1] == h && s_last[w1] == c;
        if (!merged && s_len[w] < max_labels) sc = nonan((c == s_last[w] ? s_pb[w] : s_tot[w]) + (s_tx[k] - lse));
      }
      s_c[lt] = cb_key(sc, idx);
      s_cw[lt] = w;
    } else if (lt >= next && lt < ncp - n) {   // the padding up to a multiple of 8: it precedes nothing
      s_c[n + lt] = cb_key(-INFINITY, INT_MAX);
    }
    __syncthreads();
    if (tid < nc) {
      const uint64_t me = s_c[tid];
      if (cb_key_score(me) > -INFINITY) {
        const cb_key2_t* c2 = (const cb_key2_t*)s_c;
        int r = 0;
#pragma unroll 8
        for (int j = 0; j < ncp / 2; ++j) {
          const cb_key2_t o = c2[j];
          r += o[0] > me ? 1 : 0;
          r += o[1] > me ? 1 : 0;
        }
        if (r < W) s_sel[r] = tid;
      }
    }
    __syncthreads();
    // The new state is read and written by wave 0 alone, and no other wave touches the state between the barrier
    // above and the one below: a wave's LDS accesses execute in program order, so no barrier is needed in between.
    if (wave == 0) {
      float npb = -INFINITY, npnb = -INFINITY, ntot = -INFINITY;
      int nnode = -2, nlast = -1, nlen = 0, nkoff = 0, total = 0;
      uint64_t nh = 0, nph = 0;
      const int sel = tid < W ? s_sel[tid] : -1;
      if (sel >= 0) {
        const float m = cb_key_score(s_c[s_sel[0]]);   // the frame's best tot
        const uint64_t me = s_c[sel];
        ntot = cb_key_score(me) - m;                   // (slots in score order: tot does not increase with the slot)
        if (sel >= next) {
          const int w = sel - next;
          npb = s_spb[w] - m;
          npnb = s_spnb[w] - m;
          nnode = s_node[w];
          nh = s_h[w];
          nph = s_ph[w];
          nlast = s_last[w];
          nlen = s_len[w];
        } else {
          const int idx = cb_key_idx(me), w = s_cw[sel];
          npnb = ntot;
          nnode = 1 + t * W + tid;
          nlast = idx - w * V;
          nlen = s_len[w] + 1;
          nph = s_h[w];
          nh = cb_hash(nph, nlast);
          w_trie[2 * (int64_t)(nnode - 1)] = s_node[w];
          w_trie[2 * (int64_t)(nnode - 1) + 1] = nlast;
        }
        if (more && nlast >= 0) p_xl = xn[nlast];
        if (tid == 0) off += (double)m;
      }
      // the next frame's candidate layout: the slots that may still extend, in order
      const uint64_t livem = __ballot(sel >= 0);
      const uint64_t openm = __ballot(sel >= 0 && nlen < max_labels);
      int u = 0;
      for (int w = 0; w < W; ++w) {
        if (w == tid) nkoff = total;
        if ((openm >> w) & 1) total += s_offer[u++];
      }
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");   // every lane has read the old state
      __builtin_amdgcn_wave_barrier();
      if (tid < W) {
        s_pb[tid] = npb;
        s_pnb[tid] = npnb;
        s_tot[tid] = ntot;
        s_node[tid] = nnode;
        s_h[tid] = nh;
        s_ph[tid] = nph;
        s_last[tid] = nlast;
        s_len[tid] = nlen;
        s_sel[tid] = -1;
        s_koff[tid] = nkoff;
      }
      if (tid == 0) {
        s_n = __popcll(livem);
        s_next = total;
        s_lse = p_lse;
      }
    } else if (lt < K) {
      s_tx[lt] = p_x;
      s_ti[lt] = p_i;
    }
    xb = p_xb;
    xl = p_xl;
    __syncthreads();
  }
  if (tid == 0) s_off = off;
  __syncthreads();

  // ---- results: the slots are in rank order already; walk each one's trie path back
  const int n = s_n;
  if (tid == 0) n_hyp[b] = n;
  if (tid < W) {
    const int64_t slot = (int64_t)b * W + tid;
    int64_t* out = tok + slot * max_labels;
    int l = 0;
    float sc = -INFINITY;
    if (tid < n) {
      l = s_len[tid];
      sc = (float)(s_off + (double)s_tot[tid]);
      int node = s_node[tid];
      for (int p = l - 1; p >= 0 && node > 0; --p) {
        out[p] = w_trie[2 * (int64_t)(node - 1) + 1];
        node = w_trie[2 * (int64_t)(node - 1)];
      }
    }
    for (int p = l; p < max_labels; ++p) out[p] = blank;
    len[slot] = l;
    score[slot] = sc;
  }
}

// one wave per hypothesis row
__global__ __launch_bounds__(64) void hyp_tokens_kernel(const int64_t* __restrict__ tok, int64_t ld_tok,
                                                        const int32_t* __restrict__ len,
                                                        const int32_t* __restrict__ n_hyp, int W, int L, int64_t bos,
                                                        int64_t eos, int64_t pad, int64_t ignore,
                                                        int64_t* __restrict__ dec_in, int64_t* __restrict__ dec_tgt,
                                                        float* __restrict__ mask) {
  const int r = blockIdx.x, lane = threadIdx.x;
  const bool dead = n_hyp && (r % W) >= n_hyp[r / W];
  int n = len[r];
  n = clamp_len(n, L - 1);
  n = n > ld_tok ? (int)ld_tok : n;
  const int64_t* src = tok + (int64_t)r * ld_tok;
  for (int i = lane; i < L; i += 64) {
    const int64_t o = (int64_t)r * L + i;
    if (dead) {
      dec_in[o] = pad;
      dec_tgt[o] = ignore;
      mask[o] = 0.f;
    } else {
      dec_in[o] = i == 0 ? bos : (i <= n ? src[i - 1] : pad);
      dec_tgt[o] = i < n ? src[i] : (i == n ? eos : ignore);
      mask[o] = i <= n ? 1.f : 0.f;
    }
  }
}

// one wave per sequence: the positions in order, each row's logsumexp max-subtracted
__global__ __launch_bounds__(64) void seq_logprob_kernel(const float* __restrict__ logits, int L, int V, int64_t ld,
                                                         const int64_t* __restrict__ tgt, int64_t ignore,
                                                         const int32_t* __restrict__ n_hyp, int W,
                                                         float* __restrict__ out) {
  const int r = blockIdx.x, lane = threadIdx.x;
  if (n_hyp && (r % W) >= n_hyp[r / W]) {
    if (lane == 0) out[r] = -INFINITY;
    return;
  }
  float acc = 0.f;
  for (int i = 0; i < L; ++i) {
    const int64_t tg = tgt[(int64_t)r * L + i];
    if (tg == ignore || tg < 0 || tg >= V) continue;   // (wave-uniform)
    const float* x = logits + ((int64_t)r * L + i) * ld;
    float mx = -INFINITY;
    for (int c = lane; c < V; c += 64) mx = fmaxf(mx, x[c]);
    mx = wave_max(mx);
    float sum = 0.f;
    for (int c = lane; c < V; c += 64) sum += expf(x[c] - mx);
    sum = wave_sum(sum);
    acc += (x[tg] - mx) - logf(sum);
  }
  if (lane == 0) out[r] = acc;
}

// one wave per sample: lane j holds hypothesis j
__global__ __launch_bounds__(64) void rescore_rank_kernel(const float* __restrict__ att,
                                                          const float* __restrict__ ctc, int W, float att_w,
                                                          float ctc_w, float* __restrict__ score,
                                                          int32_t* __restrict__ order) {
  const int b = blockIdx.x, lane = threadIdx.x;
  float s = -INFINITY;
  if (lane < W) {
    const float a = att[b * W + lane], c = ctc[b * W + lane];
    // a dead hypothesis (either term -inf) stays dead under a zero weight
    if (a > -INFINITY && c > -INFINITY) s = nonan(__builtin_fmaf(ctc_w, c, att_w * a));
  }
  int r = 0;
  for (int j = 0; j < W; ++j) {
    const float o = __shfl(s, j, 64);
    r += ranks_before(o, j, s, lane) ? 1 : 0;
  }
  if (lane < W) {
    score[b * W + lane] = s;
    order[b * W + r] = lane;
  }
}

}  // namespace

extern "C" int asrx_ctc_prefix_beam(const float* logits, int32_t B, int32_t T, int32_t V, int64_t ld,
                                    const int32_t* input_lengths, int32_t blank, int32_t W, int32_t max_labels,
                                    void* ws, int64_t ws_words, int64_t* tok, int32_t* len, float* score,
                                    int32_t* n_hyp, void* stream) {
  if (W < 1 || W > CB_MAXW || T <= 0 || V <= 0 || blank < 0 || blank >= V || max_labels < 1) return ASRX_ERR_ARG;
  if (B < 0 || ld < V) return ASRX_ERR_ARG;
  if (!logits || !ws || !tok || !len || !score || !n_hyp || ((uintptr_t)ws & 3) != 0) return ASRX_ERR_ARG;
  if (V > CB_MAXV || B > 65535 || (int64_t)T * W > 0x3fffffffLL) return ASRX_ERR_UNSUPPORTED;
  if (ws_words < (int64_t)B * T * (1 + 6 * W)) return ASRX_ERR_ARG;
  if (B == 0) return ASRX_OK;
  if (V <= 256)
    hipLaunchKernelGGL(ctc_prefix_beam_kernel<4>, dim3((unsigned)B), dim3(CB_THREADS), 0, (hipStream_t)stream,
                       logits, (int)T, (int)V, ld, input_lengths, (int)blank, (int)W, (int)max_labels, (float*)ws, tok,
                       len, score, n_hyp);
  else if (V <= 64 * CB_XR)
    hipLaunchKernelGGL(ctc_prefix_beam_kernel<CB_XR>, dim3((unsigned)B), dim3(CB_THREADS), 0, (hipStream_t)stream,
                       logits, (int)T, (int)V, ld, input_lengths, (int)blank, (int)W, (int)max_labels, (float*)ws, tok,
                       len, score, n_hyp);
  else
    hipLaunchKernelGGL(ctc_prefix_beam_kernel<0>, dim3((unsigned)B), dim3(CB_THREADS), 0, (hipStream_t)stream,
                       logits, (int)T, (int)V, ld, input_lengths, (int)blank, (int)W, (int)max_labels, (float*)ws, tok,
                       len, score, n_hyp);
  ASRX_CHECK_LAUNCH();
  return ASRX_OK;
}

extern "C" int asrx_hyp_tokens(const int64_t* tok, int64_t ld_tok, const int32_t* len, const int32_t* n_hyp, int32_t B,
                               int32_t W, int32_t L, int64_t bos, int64_t eos, int64_t pad, int64_t ignore,
                               int64_t* dec_in, int64_t* dec_tgt, float* mask, void* stream) {
  if (!tok || !len || !dec_in || !dec_tgt || !mask) return ASRX_ERR_ARG;
  if (B < 0 || W < 1 || W > CB_MAXW || L < 1 || ld_tok < 1) return ASRX_ERR_ARG;
  if ((int64_t)B * W > 0x7fffffffLL) return ASRX_ERR_UNSUPPORTED;
  if (B == 0) return ASRX_OK;
  hipLaunchKernelGGL(hyp_tokens_kernel, dim3((unsigned)(B * W)), dim3(64), 0, (hipStream_t)stream, tok, ld_tok, len,
                     n_hyp, (int)W, (int)L, bos, eos, pad, ignore, dec_in, dec_tgt, mask);
  ASRX_CHECK_LAUNCH();
  return ASRX_OK;
}

extern "C" int asrx_seq_logprob(const float* logits, int32_t N, int32_t L, int32_t V, int64_t ld, const int64_t* tgt,
                                int64_t ignore, const int32_t* n_hyp, int32_t W, float* out, void* stream) {
  if (!logits || !tgt || !out || N < 0 || L < 1 || V < 1 || ld < V) return ASRX_ERR_ARG;
  if (n_hyp && (W < 1 || N % W != 0)) return ASRX_ERR_ARG;
  if (N == 0) return ASRX_OK;
  hipLaunchKernelGGL(seq_logprob_kernel, dim3((unsigned)N), dim3(64), 0, (hipStream_t)stream, logits, (int)L, (int)V,
                     ld, tgt, ignore, n_hyp, (int)(n_hyp ? W : 1), out);
  ASRX_CHECK_LAUNCH();
  return ASRX_OK;
}

extern "C" int asrx_rescore_rank(const float* att, const float* ctc, int32_t B, int32_t W, float att_weight,
                                 float ctc_weight, float* score, int32_t* order, void* stream) {
  if (!att || !ctc || !score || !order || B < 0 || W < 1 || W > CB_MAXW) return ASRX_ERR_ARG;
  if (att_weight != att_weight || ctc_weight != ctc_weight) return ASRX_ERR_ARG;
  if ((int64_t)B * W > 0x7fffffffLL) return ASRX_ERR_UNSUPPORTED;
  if (B == 0) return ASRX_OK;
  hipLaunchKernelGGL(rescore_rank_kernel, dim3((unsigned)B), dim3(64), 0, (hipStream_t)stream, att, ctc, (int)W,
                     att_weight, ctc_weight, score, order);
  ASRX_CHECK_LAUNCH();
  return ASRX_OK;
}
