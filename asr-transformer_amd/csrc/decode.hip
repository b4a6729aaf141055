// Beam-search decoding on the device: the per-sample top-W over the W x V continuation scores of one decode step
// (asrx_beam_step; asrx_beam_step_joint adds a weighted second score per candidate, the CTC prefix score of
// ctc_prefix.hip) and the reorder of the self-attention K/V caches by the chosen parents (asrx_gather_rows).
// The reference decodes greedily only (model.py:125-151); these two serve Decoder.beam_search.
#include <limits.h>

#include "common.h"

// ---- asrx_beam_step
//
// One workgroup of 256 threads per sample.  The candidates of a sample are ordered by (score descending, flat index
// w*V+v ascending), a total order once NaN scores are read as -inf, so the j-th best is "the best candidate that
// comes strictly after the (j-1)-th": every round is a workgroup-wide arg-max over immutable candidates, nothing is
// marked as taken.  Candidates live in LDS when W*V floats fit; otherwise each round forms them again from the
// logits (L2-resident: W*V*4 B per sample) with the same expression, so both paths select the same slots.
#define BEAM_THREADS 256
#define BEAM_WAVES (BEAM_THREADS / 64)
#define BEAM_MAXW 16
#define BEAM_LDS_CAND 16128   // floats of dynamic LDS (63 KiB) next to the ~0.3 KiB of static exchange words
#define BEAM_MAXV (1 << 20)

struct BeamBest {
  float s;
  int i;
};
ASRX_DEV float beam_cand(float score, float logit, float lse) { return nonan(score + (logit - lse)); }

// the joint candidate: score + att_w * (logit - lse) + ext_w * extra.  The multiply-adds are explicit so that the LDS
// and the re-read path round alike whatever the compiler would contract; att_w = 1, ext_w = 0 with extra = 0 is
// beam_cand bit for bit.
ASRX_DEV float beam_cand_joint(float score, float logit, float lse, float att_w, float ext_w, float extra) {
  return nonan(__builtin_fmaf(ext_w, extra, __builtin_fmaf(att_w, logit - lse, score)));
}

struct BeamExtra {
  const float* extra;   // [B*W][ld]: a second score per candidate (JOINT only)
  int64_t ld;
  float att_w, ext_w;
};

template <bool LDS, bool JOINT>
__global__ __launch_bounds__(BEAM_THREADS) void beam_step_kernel(
    const float* __restrict__ logits, int W, int V, int64_t ld, BeamExtra ex, const float* __restrict__ score_in,
    const uint8_t* __restrict__ fin_in, const int32_t* __restrict__ len_in, int eos, float* __restrict__ score_out,
    int64_t* __restrict__ tok_out, int64_t* __restrict__ cur, int32_t* __restrict__ parent_out,
    int32_t* __restrict__ src_row_out, uint8_t* __restrict__ fin_out, int32_t* __restrict__ len_out,
    int32_t* __restrict__ n_live) {
  extern __shared__ __attribute__((aligned(16))) float cand[];   // [W][V], LDS path only
  __shared__ float s_lse[BEAM_MAXW];
  __shared__ float s_score[BEAM_MAXW];
  __shared__ int s_fin[BEAM_MAXW];
  __shared__ float s_rs[2][BEAM_WAVES];
  __shared__ int s_ri[2][BEAM_WAVES];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t row0 = (int64_t)blockIdx.x * W;
  const float* x0 = logits + row0 * ld;
  const float* e0 = JOINT ? ex.extra + row0 * ex.ld : nullptr;

  // max-subtracted logsumexp of each live beam's row, one wave per beam
  for (int w = wave; w < W; w += BEAM_WAVES) {
    const int fin = fin_in[row0 + w] != 0;
    float lse = 0.f;
    if (!fin) {
      const float* x = x0 + (int64_t)w * ld;
      float mx = -INFINITY;
      bool nan = false;
      for (int c = lane; c < V; c += 64) {
        const float v = x[c];
        nan |= v != v;
        mx = fmaxf(mx, v);
      }
      mx = wave_max(mx);
      float sum = 0.f;
      for (int c = lane; c < V; c += 64) sum += expf(x[c] - mx);
      sum = wave_sum(sum);
      lse = mx + logf(sum);
      if (__any(nan)) lse = __builtin_nanf("");   // fmaxf drops a NaN logit; the row's logsumexp is NaN all the same
    }
    if (lane == 0) {
      s_lse[w] = lse;
      s_score[w] = score_in[row0 + w];
      s_fin[w] = fin;
    }
  }
  __syncthreads();

  const int n = W * V;
  if (LDS) {
    // a finished beam keeps one candidate, (w, eos) at its score; the others do not exist (NaN marks the gap)
    for (int i = tid; i < n; i += BEAM_THREADS) {
      const int w = i / V, v = i - w * V;
      float c;
      if (s_fin[w]) {
        const float s = s_score[w];
        c = v == eos ? nonan(s) : __builtin_nanf("");
      } else {
        c = JOINT ? beam_cand_joint(s_score[w], x0[(int64_t)w * ld + v], s_lse[w], ex.att_w, ex.ext_w,
                                    e0[(int64_t)w * ex.ld + v])
                  : beam_cand(s_score[w], x0[(int64_t)w * ld + v], s_lse[w]);
      }
      cand[i] = c;
    }
    __syncthreads();
  }

  float ps = INFINITY;   // the previous round's pick: the first round takes anything after (+inf, -1)
  int pi = -1;
  int live = 0;
  for (int j = 0; j < W; ++j) {
    float bs = -INFINITY;
    int bi = INT_MAX;
    if (LDS) {
      for (int i = tid; i < n; i += BEAM_THREADS) {
        const float c = cand[i];
        if (c == c && ranks_before(ps, pi, c, i) && ranks_before(c, i, bs, bi)) { bs = c; bi = i; }
      }
    } else {
      for (int w = 0; w < W; ++w) {
        const float sc = s_score[w];
        if (s_fin[w]) {
          if (tid == 0) {
            const float c = nonan(sc);
            const int i = w * V + eos;
            if (ranks_before(ps, pi, c, i) && ranks_before(c, i, bs, bi)) { bs = c; bi = i; }
          }
          continue;
        }
        const float* x = x0 + (int64_t)w * ld;
        const float* e = JOINT ? e0 + (int64_t)w * ex.ld : nullptr;
        const float lse = s_lse[w];
        for (int v = tid; v < V; v += BEAM_THREADS) {
          const float c = JOINT ? beam_cand_joint(sc, x[v], lse, ex.att_w, ex.ext_w, e[v]) : beam_cand(sc, x[v], lse);
          const int i = w * V + v;
          if (ranks_before(ps, pi, c, i) && ranks_before(c, i, bs, bi)) { bs = c; bi = i; }
        }
      }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float os = __shfl_xor(bs, o, 64);
      const int oi = __shfl_xor(bi, o, 64);
      if (ranks_before(os, oi, bs, bi)) { bs = os; bi = oi; }
    }
    const int pp = j & 1;   // two exchange slots: round j+1 writes the other one, so one barrier per round
    if (lane == 0) {
      s_rs[pp][wave] = bs;
      s_ri[pp][wave] = bi;
    }
    __syncthreads();
    bs = s_rs[pp][0];
    bi = s_ri[pp][0];
#pragma unroll
    for (int k = 1; k < BEAM_WAVES; ++k) {
      const float os = s_rs[pp][k];
      const int oi = s_ri[pp][k];
      if (ranks_before(os, oi, bs, bi)) { bs = os; bi = oi; }
    }
    // every sample has at least W candidates (V per live beam, one per finished beam), so bi is a real index
    ps = bs;
    pi = bi;
    if (tid == 0) {
      const int parent = bi / V, tok = bi - parent * V;
      const int64_t slot = row0 + j;
      const int pfin = s_fin[parent];
      const int fin = pfin | (tok == eos);
      score_out[slot] = bs;
      tok_out[slot] = tok;
      if (cur) cur[slot] = tok;
      parent_out[slot] = parent;
      src_row_out[slot] = (int32_t)(row0 + parent);
      fin_out[slot] = (uint8_t)fin;
      len_out[slot] = len_in[row0 + parent] + (pfin ? 0 : 1);
      live += !fin;
    }
  }
  if (tid == 0 && n_live && live) atomicAdd(n_live, live);
}

template <bool JOINT>
static int beam_step_launch(const float* logits, int32_t B, int32_t W, int32_t V, int64_t ld, BeamExtra ex,
                            const float* score_in, const uint8_t* fin_in, const int32_t* len_in, int64_t eos,
                            float* score_out, int64_t* tok_out, int64_t* cur, int32_t* parent_out,
                            int32_t* src_row_out, uint8_t* fin_out, int32_t* len_out, int32_t* n_live, void* stream) {
  if (!logits || !score_in || !fin_in || !len_in || !score_out || !tok_out || !parent_out || !src_row_out ||
      !fin_out || !len_out)
    return ASRX_ERR_ARG;
  if (B < 0 || W < 1 || W > BEAM_MAXW || V < 1 || ld < V || eos < 0 || eos >= V) return ASRX_ERR_ARG;
  if ((const void*)score_in == (const void*)score_out || (const void*)fin_in == (const void*)fin_out ||
      (const void*)len_in == (const void*)len_out)
    return ASRX_ERR_ARG;
  if (V > BEAM_MAXV || (int64_t)B * W > INT_MAX) return ASRX_ERR_UNSUPPORTED;
  if (B == 0) return ASRX_OK;
  hipStream_t st = (hipStream_t)stream;
  const int n = W * V;
  if (n <= BEAM_LDS_CAND)
    hipLaunchKernelGGL((beam_step_kernel<true, JOINT>), dim3((unsigned)B), dim3(BEAM_THREADS),
                       (size_t)n * sizeof(float), st, logits, (int)W, (int)V, ld, ex, score_in, fin_in, len_in,
                       (int)eos, score_out, tok_out, cur, parent_out, src_row_out, fin_out, len_out, n_live);
  else
    hipLaunchKernelGGL((beam_step_kernel<false, JOINT>), dim3((unsigned)B), dim3(BEAM_THREADS), 0, st, logits, (int)W,
                       (int)V, ld, ex, score_in, fin_in, len_in, (int)eos, score_out, tok_out, cur, parent_out,
                       src_row_out, fin_out, len_out, n_live);
  ASRX_CHECK_LAUNCH();
  return ASRX_OK;
}

extern "C" int asrx_beam_step(const float* logits, int32_t B, int32_t W, int32_t V, int64_t ld, const float* score_in,
                              const uint8_t* fin_in, const int32_t* len_in, int64_t eos, float* score_out,
                              int64_t* tok_out, int64_t* cur, int32_t* parent_out, int32_t* src_row_out,
                              uint8_t* fin_out, int32_t* len_out, int32_t* n_live, void* stream) {
  return beam_step_launch<false>(logits, B, W, V, ld, BeamExtra{nullptr, 0, 1.f, 0.f}, score_in, fin_in, len_in, eos,
                                 score_out, tok_out, cur, parent_out, src_row_out, fin_out, len_out, n_live, stream);
}

extern "C" int asrx_beam_step_joint(const float* logits, int32_t B, int32_t W, int32_t V, int64_t ld,
                                    const float* extra, int64_t ld_extra, float att_weight, float extra_weight,
                                    const float* score_in, const uint8_t* fin_in, const int32_t* len_in, int64_t eos,
                                    float* score_out, int64_t* tok_out, int64_t* cur, int32_t* parent_out,
                                    int32_t* src_row_out, uint8_t* fin_out, int32_t* len_out, int32_t* n_live,
                                    void* stream) {
  if (!extra || ld_extra < V || att_weight != att_weight || extra_weight != extra_weight) return ASRX_ERR_ARG;
  return beam_step_launch<true>(logits, B, W, V, ld, BeamExtra{extra, ld_extra, att_weight, extra_weight}, score_in,
                                fin_in, len_in, eos, score_out, tok_out, cur, parent_out, src_row_out, fin_out,
                                len_out, n_live, stream);
}

// ---- asrx_gather_rows
//
// dst[o][r][0:count) = src[o][index[r]][0:count): grid (chunks of a row, rows, outer), T = the widest unit the
// alignment of bases, strides and count allows (16 B, else one element).  A row whose index lies outside
// [0, rows) is left as it is.
template <typename T>
__global__ __launch_bounds__(256) void gather_rows_kernel(const T* __restrict__ src, T* __restrict__ dst,
                                                          const int32_t* __restrict__ index, int rows, int64_t count,
                                                          int64_t row_stride, int64_t outer_stride) {
  const int r = blockIdx.y;
  const int s = index[r];
  if (s < 0 || s >= rows) return;
  const int64_t ob = (int64_t)blockIdx.z * outer_stride;
  const T* __restrict__ sp = src + ob + (int64_t)s * row_stride;
  T* __restrict__ dp = dst + ob + (int64_t)r * row_stride;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < count; i += (int64_t)gridDim.x * 256) dp[i] = sp[i];
}

template <typename T>
static int gather_launch(const void* src, void* dst, const int32_t* index, int outer, int rows, int64_t count,
                         int64_t row_stride, int64_t outer_stride, hipStream_t st) {
  const int64_t chunks = (count + 1023) / 1024;   // up to 4 units per thread
  const dim3 grid((unsigned)(chunks < 64 ? chunks : 64), (unsigned)rows, (unsigned)outer);
  hipLaunchKernelGGL((gather_rows_kernel<T>), grid, dim3(256), 0, st, (const T*)src, (T*)dst, index, rows, count,
                     row_stride, outer_stride);
  ASRX_CHECK_LAUNCH();
  return ASRX_OK;
}

extern "C" int asrx_gather_rows(const void* src, void* dst, const int32_t* index, int32_t esize, int32_t outer,
                                int32_t rows, int64_t count, int64_t row_stride, int64_t outer_stride,
                                void* stream) {
  if (!src || !dst || !index || src == dst) return ASRX_ERR_ARG;
  if (esize != 2 && esize != 4) return ASRX_ERR_ARG;
  if (outer < 0 || rows < 0 || count < 0 || row_stride < count) return ASRX_ERR_ARG;
  if (outer > 1 && outer_stride < (int64_t)rows * row_stride) return ASRX_ERR_ARG;
  if (((uintptr_t)src | (uintptr_t)dst) % (uintptr_t)esize) return ASRX_ERR_ARG;
  if (outer == 0 || rows == 0 || count == 0) return ASRX_OK;
  if (outer > 65535 || rows > 65535) return ASRX_ERR_UNSUPPORTED;
  // the two buffers share one layout; their extents must not overlap
  const int64_t extent = ((int64_t)(outer - 1) * outer_stride + (int64_t)(rows - 1) * row_stride + count) * esize;
  const uintptr_t a = (uintptr_t)src, b = (uintptr_t)dst;
  if (a < b ? a + (uintptr_t)extent > b : b + (uintptr_t)extent > a) return ASRX_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  const int64_t per16 = 16 / esize;
  const bool wide = (a | b) % 16 == 0 && row_stride % per16 == 0 && outer_stride % per16 == 0 && count % per16 == 0;
  if (wide)
    return gather_launch<v4u_t>(src, dst, index, outer, rows, count / per16, row_stride / per16,
                                outer_stride / per16, st);
  if (esize == 2) return gather_launch<uint16_t>(src, dst, index, outer, rows, count, row_stride, outer_stride, st);
  return gather_launch<uint32_t>(src, dst, index, outer, rows, count, row_stride, outer_stride, st);
}
