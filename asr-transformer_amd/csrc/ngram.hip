// Back-off n-gram language model on the device, for shallow fusion in beam search and for second-pass rescoring.
// C-ABI: asrx_ngram_score, asrx_ngram_advance, asrx_ngram_seq_logprob (include/asrx.h); the selection that consumes
// the scores is asrx_beam_step_joint (decode.hip), whose `extra` matrix asrx_ngram_score writes directly.
//
// The table is a forward trie in breadth-first order: node 0 the empty context, nodes 1 .. V the unigrams (token v is
// node 1 + v, every id present), higher orders level by level, so the children of node i are the nodes
// [first_child[i], first_child[i + 1]), contiguous and sorted by ascending token.  A hypothesis carries order - 1 node
// numbers: ctx[k - 1] spells its last k tokens, or is -1 where that k-gram is not in the table.  The orders are looked
// up independently of each other ("a b c" may exist without "b c").  With k* the longest context that has the word,
//   lm(v) = logp[child(ctx[k* - 1], v)] + sum over the valid j > k* of backoff[ctx[j - 1]]     (k* = 0: logp[1 + v])
// added in ascending j in fp32 (ngram_chain): one rounding sequence in all three kernels.
//
// The table lives in device memory and the host never reads it, so every index that comes out of it is checked before
// it is used: a context outside [0, n_nodes) reads as -1, a child range is clamped to [0, n_nodes], a token outside
// [0, V) is skipped.  No atomics, fixed summation orders: the same inputs give the same bits.
#include "ctc_common.h"

namespace {

constexpr int NG_MAXCTX = ASRX_NGRAM_MAX_ORDER - 1;
constexpr int NG_THREADS = 256;
constexpr int NG_LDS_V = ASRX_NGRAM_LDS_V;   // longest row asrx_ngram_score keeps in LDS (32 KiB)
constexpr int NG_MAXL = 4096;                // longest row of asrx_ngram_seq_logprob (two LDS arrays of 16 KiB)

struct NgramTable {
  const int32_t* first_child;
  const int32_t* token;
  const float* logp;
  const float* backoff;
  int n_nodes, order, V;
};

// the child range of a node, safe against any table contents (node in [0, n_nodes))
ASRX_DEV void ngram_range(const NgramTable& T, int node, int& lo, int& hi) {
  lo = clamp_len(T.first_child[node], T.n_nodes);
  hi = clamp_len(T.first_child[node + 1], T.n_nodes);
}

ASRX_DEV int ngram_valid(const NgramTable& T, int node) { return node >= 0 && node < T.n_nodes ? node : -1; }

// the child of `node` with token v (binary search over the sorted child list), -1 if there is none
ASRX_DEV int ngram_child(const NgramTable& T, int node, int v) {
  if (node < 0 || node >= T.n_nodes) return -1;
  int lo, hi;
  ngram_range(T, node, lo, hi);
  const int end = hi;
  while (lo < hi) {
    const int mid = lo + ((hi - lo) >> 1);
    if (T.token[mid] < v) lo = mid + 1;
    else hi = mid;
  }
  return lo < end && T.token[lo] == v ? lo : -1;
}

// the back-off weights of a slot's contexts: bo[j - 1] = backoff[ctx[j - 1]], 0 where the context is absent
ASRX_DEV void ngram_backoffs(const NgramTable& T, const int (&node)[NG_MAXCTX], float (&bo)[NG_MAXCTX]) {
#pragma unroll
  for (int j = 0; j < NG_MAXCTX; ++j) bo[j] = j < T.order - 1 && node[j] >= 0 ? T.backoff[node[j]] : 0.f;
}

// acc + the back-off weights of the contexts longer than k, in ascending order
ASRX_DEV float ngram_chain(float acc, const float (&bo)[NG_MAXCTX], int k) {
#pragma unroll
  for (int j = 0; j < NG_MAXCTX; ++j)
    if (j >= k) acc += bo[j];
  return acc;
}

// ---------------------------------------------------------------------------------------------- score
// One workgroup per slot.  The row of lm(v) is built level by level: the unigram level fills every column, then each
// order whose context exists overwrites the columns of its children, a workgroup barrier between two levels (a column
// written by two orders ends with the longer one's value whatever the thread timing).  LDS_ROW: the row stands in LDS
// and `out` is written once, coalesced; otherwise the `out` row itself is the accumulator and the last pass rewrites
// it in place (each thread its own columns).
template <bool LDS_ROW>
__global__ __launch_bounds__(NG_THREADS) void ngram_score_kernel(NgramTable T, const int32_t* __restrict__ ctx,
                                                                 const float* base, int64_t ld_base,
                                                                 float base_weight, float lm_weight, float bonus,
                                                                 float* out, int64_t ld_out) {
  __shared__ float s_row[LDS_ROW ? NG_LDS_V : 1];
  const int64_t r = blockIdx.x;
  const int tid = threadIdx.x;
  float* orow = out + r * ld_out;
  float* row = LDS_ROW ? s_row : orow;
  int node[NG_MAXCTX];
  float bo[NG_MAXCTX];
#pragma unroll
  for (int j = 0; j < NG_MAXCTX; ++j) node[j] = j < T.order - 1 ? ngram_valid(T, ctx[r * (T.order - 1) + j]) : -1;
  ngram_backoffs(T, node, bo);

  for (int v = tid; v < T.V; v += NG_THREADS) row[v] = ngram_chain(T.logp[1 + v], bo, 0);
  __syncthreads();
#pragma unroll
  for (int k = 1; k <= NG_MAXCTX; ++k) {
    if (k >= T.order) break;        // (uniform: the barriers below are met by all threads or by none)
    if (node[k - 1] >= 0) {
      int lo, hi;
      ngram_range(T, node[k - 1], lo, hi);
      for (int i = lo + tid; i < hi; i += NG_THREADS) {
        const int v = T.token[i];
        if (v >= 0 && v < T.V) row[v] = ngram_chain(T.logp[i], bo, k);
      }
    }
    __syncthreads();
  }
  const float* brow = base ? base + r * ld_base : nullptr;
  for (int v = tid; v < T.V; v += NG_THREADS) {
    float o = bonus;
    if (lm_weight != 0.f) o = __builtin_fmaf(lm_weight, row[v], o);
    if (brow) o = __builtin_fmaf(base_weight, brow[v], o);
    orow[v] = o;
  }
}

// ---------------------------------------------------------------------------------------------- advance
// One thread per (slot, context length k = 1 .. order - 1).
__global__ __launch_bounds__(NG_THREADS) void ngram_advance_kernel(NgramTable T, int64_t R, int W, int eos,
                                                                   const int32_t* __restrict__ parent,
                                                                   const int64_t* __restrict__ tok,
                                                                   const uint8_t* __restrict__ fin_prev,
                                                                   const int32_t* __restrict__ ctx_in,
                                                                   int32_t* __restrict__ ctx_out) {
  const int nctx = T.order - 1;
  const int64_t e = (int64_t)blockIdx.x * NG_THREADS + threadIdx.x;
  if (e >= R * nctx) return;
  const int64_t slot = e / nctx;
  const int k = (int)(e % nctx) + 1;
  const int64_t b = slot / W;
  const int64_t ps = b * W + clamp_len(parent[slot], W - 1);
  const int64_t tk = tok[slot];
  const int32_t* src = ctx_in + ps * nctx;
  int res;
  if (fin_prev[ps] != 0 || tk == (int64_t)eos) {
    res = src[k - 1];
  } else if (tk < 0 || tk >= T.V) {
    res = -1;
  } else if (k == 1) {
    res = 1 + (int)tk;
  } else {
    res = ngram_child(T, src[k - 2], (int)tk);
  }
  ctx_out[slot * nctx + (k - 1)] = res;
}

// ---------------------------------------------------------------------------------------------- sequences
// One workgroup per sequence.  Wave 0 packs the scored tokens of the row into LDS (ballot scan, position order); then
// every thread takes packed positions i = tid, tid + 256, ...: the contexts of position i are walked from the unigram
// of each history start (no state is carried from position to position, so the positions are independent), the word
// is looked up as in the score kernel, and the terms are summed by one thread in position order.
__global__ __launch_bounds__(NG_THREADS) void ngram_seq_kernel(NgramTable T, const int64_t* __restrict__ tgt,
                                                               int64_t ld_tgt, int L, int64_t ignore, int bos,
                                                               const int32_t* __restrict__ n_hyp, int W,
                                                               const float* __restrict__ add, float add_scale,
                                                               float lm_weight, float bonus,
                                                               float* __restrict__ lm_out, float* __restrict__ out) {
  __shared__ int s_tok[NG_MAXL];
  __shared__ float s_val[NG_MAXL];
  __shared__ int s_n;
  const int64_t n = blockIdx.x;
  const int tid = threadIdx.x;
  if (n_hyp && (int)(n % W) >= n_hyp[n / W]) {   // (uniform per workgroup)
    if (tid == 0) {
      lm_out[n] = -INFINITY;
      out[n] = -INFINITY;
    }
    return;
  }
  const int64_t* row = tgt + n * ld_tgt;
  if (tid < 64) {
    int cnt = 0;
    for (int i0 = 0; i0 < L; i0 += 64) {
      const int i = i0 + tid;
      const int64_t t = i < L ? row[i] : ignore;
      const bool ok = i < L && t != ignore && t >= 0 && t < T.V;
      const uint64_t m = __ballot(ok);
      if (ok) s_tok[cnt + __popcll(m & ((1ull << tid) - 1ull))] = (int)t;
      cnt += __popcll(m);
    }
    if (tid == 0) s_n = cnt;
  }
  __syncthreads();
  const int cnt = s_n;
  const int hb = bos >= 0 && bos < T.V ? 1 : 0;   // the history starts with the sentence-start token
  for (int i = tid; i < cnt; i += NG_THREADS) {
    int node[NG_MAXCTX];
#pragma unroll
    for (int k = 1; k <= NG_MAXCTX; ++k) {
      int nd = -1;
      if (k < T.order && k <= i + hb) {
        // history positions i - k .. i - 1 (position -1 = the sentence start)
        const int p0 = i - k;
        nd = 1 + (p0 < 0 ? bos : s_tok[p0]);
        for (int m = 1; m < k && nd >= 0; ++m) nd = ngram_child(T, nd, s_tok[p0 + m]);
      }
      node[k - 1] = nd;
    }
    float bo[NG_MAXCTX];
    ngram_backoffs(T, node, bo);
    const int w = s_tok[i];
    int ks = 0, hit = 1 + w;
#pragma unroll
    for (int k = NG_MAXCTX; k >= 1; --k) {
      if (ks == 0 && k < T.order && node[k - 1] >= 0) {
        const int c = ngram_child(T, node[k - 1], w);
        if (c >= 0) {
          ks = k;
          hit = c;
        }
      }
    }
    s_val[i] = ngram_chain(T.logp[hit], bo, ks);
  }
  __syncthreads();
  if (tid == 0) {
    float lm = 0.f;
    for (int i = 0; i < cnt; ++i) lm += s_val[i];
    lm_out[n] = lm;
    float o = bonus * (float)cnt;
    if (lm_weight != 0.f) o = __builtin_fmaf(lm_weight, lm, o);
    if (add) o = __builtin_fmaf(add_scale, add[n], o);
    out[n] = o;
  }
}

bool finite(float x) { return x - x == 0.f; }

bool overlap(const void* a, int64_t abytes, const void* b, int64_t bbytes) {
  const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
  return x < y ? x + (uintptr_t)abytes > y : y + (uintptr_t)bbytes > x;
}

// the table arguments every entry point takes; the unigram level is dense, so n_nodes >= 1 + V
int check_table(const int32_t* first_child, const int32_t* token, const float* logp, const float* backoff,
                int32_t n_nodes, int32_t order, int32_t V) {
  if (!first_child || !token || !logp || !backoff) return ASRX_ERR_ARG;
  if (order < 1 || order > ASRX_NGRAM_MAX_ORDER || V < 1 || n_nodes <= V) return ASRX_ERR_ARG;
  if (V > (1 << 20)) return ASRX_ERR_UNSUPPORTED;
  return ASRX_OK;
}

}  // namespace

extern "C" int asrx_ngram_score(const int32_t* first_child, const int32_t* token, const float* logp,
                                const float* backoff, int32_t n_nodes, int32_t order, int32_t V, const int32_t* ctx,
                                int32_t R, const float* base, int64_t ld_base, float base_weight, float lm_weight,
                                float bonus, float* out, int64_t ld_out, void* stream) {
  if (const int rc = check_table(first_child, token, logp, backoff, n_nodes, order, V)) return rc;
  if (R < 0 || !ctx || !out || ld_out < V) return ASRX_ERR_ARG;
  if (!finite(base_weight) || !finite(lm_weight) || !finite(bonus)) return ASRX_ERR_ARG;
  if (base && ld_base < V) return ASRX_ERR_ARG;
  if (R == 0) return ASRX_OK;
  if (base && overlap(out, ((int64_t)(R - 1) * ld_out + V) * (int64_t)sizeof(float), base,
                      ((int64_t)(R - 1) * ld_base + V) * (int64_t)sizeof(float)))
    return ASRX_ERR_ARG;
  if (base_weight == 0.f) base = nullptr;   // a zero weight drops the term: no 0 * -inf
  const NgramTable T{first_child, token, logp, backoff, (int)n_nodes, (int)order, (int)V};
  hipStream_t st = (hipStream_t)stream;
  if (V <= NG_LDS_V)
    hipLaunchKernelGGL(ngram_score_kernel<true>, dim3((unsigned)R), dim3(NG_THREADS), 0, st, T, ctx, base, ld_base,
                       base_weight, lm_weight, bonus, out, ld_out);
  else
    hipLaunchKernelGGL(ngram_score_kernel<false>, dim3((unsigned)R), dim3(NG_THREADS), 0, st, T, ctx, base, ld_base,
                       base_weight, lm_weight, bonus, out, ld_out);
  ASRX_CHECK_LAUNCH();
  return ASRX_OK;
}

extern "C" int asrx_ngram_advance(const int32_t* first_child, const int32_t* token, const float* logp,
                                  const float* backoff, int32_t n_nodes, int32_t order, int32_t V, int32_t B, int32_t W,
                                  int32_t eos, const int32_t* parent, const int64_t* tok, const uint8_t* fin_prev,
                                  const int32_t* ctx_in, int32_t* ctx_out, void* stream) {
  if (const int rc = check_table(first_child, token, logp, backoff, n_nodes, order, V)) return rc;
  if (B < 0 || W < 1 || eos < 0 || eos >= V) return ASRX_ERR_ARG;
  if (!parent || !tok || !fin_prev || !ctx_in || !ctx_out) return ASRX_ERR_ARG;
  if ((int64_t)B * W > 0x7fffffffLL / ASRX_NGRAM_MAX_ORDER) return ASRX_ERR_UNSUPPORTED;
  if (B == 0) return ASRX_OK;
  const int64_t R = (int64_t)B * W, elems = R * (order - 1);
  const int64_t bytes = elems * (int64_t)sizeof(int32_t);
  if (ctx_in == ctx_out || overlap(ctx_in, bytes, ctx_out, bytes)) return ASRX_ERR_ARG;
  if (elems == 0) return ASRX_OK;   // a unigram model has no state
  const NgramTable T{first_child, token, logp, backoff, (int)n_nodes, (int)order, (int)V};
  hipLaunchKernelGGL(ngram_advance_kernel, dim3((unsigned)((elems + NG_THREADS - 1) / NG_THREADS)), dim3(NG_THREADS),
                     0, (hipStream_t)stream, T, R, (int)W, (int)eos, parent, tok, fin_prev, ctx_in, ctx_out);
  ASRX_CHECK_LAUNCH();
  return ASRX_OK;
}

extern "C" int asrx_ngram_seq_logprob(const int32_t* first_child, const int32_t* token, const float* logp,
                                      const float* backoff, int32_t n_nodes, int32_t order, int32_t V,
                                      const int64_t* tgt, int64_t ld_tgt, int32_t N, int32_t L, int64_t ignore,
                                      int32_t bos, const int32_t* n_hyp, int32_t W, const float* add, float add_scale,
                                      float lm_weight, float bonus, float* lm_out, float* out, void* stream) {
  if (const int rc = check_table(first_child, token, logp, backoff, n_nodes, order, V)) return rc;
  if (!tgt || !lm_out || !out || N < 0 || L < 1 || ld_tgt < L || bos < -1 || bos >= V) return ASRX_ERR_ARG;
  if (n_hyp && (W < 1 || N % W != 0)) return ASRX_ERR_ARG;
  if (!finite(add_scale) || !finite(lm_weight) || !finite(bonus)) return ASRX_ERR_ARG;
  if (L > NG_MAXL) return ASRX_ERR_UNSUPPORTED;
  if (N == 0) return ASRX_OK;
  if (add_scale == 0.f) add = nullptr;
  const NgramTable T{first_child, token, logp, backoff, (int)n_nodes, (int)order, (int)V};
  hipLaunchKernelGGL(ngram_seq_kernel, dim3((unsigned)N), dim3(NG_THREADS), 0, (hipStream_t)stream, T, tgt, ld_tgt,
                     (int)L, ignore, (int)bos, n_hyp, (int)(n_hyp ? W : 1), add, add_scale, lm_weight, bonus, lm_out,
                     out);
  ASRX_CHECK_LAUNCH();
  return ASRX_OK;
}
