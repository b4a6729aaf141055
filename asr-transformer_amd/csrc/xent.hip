// Label-smoothed cross-entropy over any vocabulary up to 2^20 (asrx_cross_entropy_ls): the semantics of
// torch.nn.functional.cross_entropy(x, t, ignore_index=, label_smoothing=eps), mean reduction, with the gradient, the
// row argmax and the perplexity / accuracy statistics from the same read of the logits.
//
//   count launch   n = #rows with target != ignore_index                      (1 workgroup)
//   rows launch    per row: (max, first argmax), sum exp, sum (x - max) -> lse, nll, smoothed loss, dlogits
//                    ld <= 16384: the row is read once and kept in registers (xent_rows_kernel)
//                    longer:      pass one keeps an online max / sum, pass two re-reads the row for the gradient
//                                 (xent_stream_kernel; one workgroup's row is at most 4 MiB, the re-read hits L2)
//   final launch   the three row vectors summed in a fixed order -> loss, stats  (1 workgroup; no float atomics)
//
// VEC = true: ld % 4 == 0 and 16-B aligned bases, 16-B loads and 8-B (bf16) / 16-B (fp32) stores; VEC = false: the
// same arithmetic on 4-B loads and 2-B / 4-B stores.  Columns [V, ld) of the logits are never read.
#include "common.h"

namespace {

constexpr int XENT_MAXV = 1 << 20;        // the decoders' limit (BEAM_MAXV, CB_MAXV)
constexpr int XENT_REG_MAXLD = 16384;     // longest register-resident row: 16 float4 per thread of 256

// ws: [0, rows) row loss, [rows, 2 rows) row nll, [2 rows, 3 rows) 1 where argmax == target, [3 rows] = n
__global__ __launch_bounds__(256) void xent_count_kernel(const int64_t* tgt, int64_t rows, int64_t ignore, float* ws) {
  __shared__ int red[256];
  int c = 0;
  for (int64_t r = threadIdx.x; r < rows; r += 256) c += tgt[r] != ignore ? 1 : 0;
  red[threadIdx.x] = c;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0) ws[3 * rows] = (float)red[0];
}

__global__ __launch_bounds__(256) void xent_final_kernel(const float* ws, int64_t rows, float* loss, float* stats) {
  __shared__ float red[3][256];
  float s0 = 0.f, s1 = 0.f, s2 = 0.f;
  for (int64_t r = threadIdx.x; r < rows; r += 256) {
    s0 += ws[r];
    s1 += ws[rows + r];
    s2 += ws[2 * rows + r];
  }
  red[0][threadIdx.x] = s0;
  red[1][threadIdx.x] = s1;
  red[2][threadIdx.x] = s2;
  __syncthreads();
  for (int k = 128; k > 0; k >>= 1) {
    if (threadIdx.x < k) {
      red[0][threadIdx.x] += red[0][threadIdx.x + k];
      red[1][threadIdx.x] += red[1][threadIdx.x + k];
      red[2][threadIdx.x] += red[2][threadIdx.x + k];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const float n = ws[3 * rows];
    loss[0] = n > 0.f ? red[0][0] / n : 0.f;
    if (stats) {
      stats[0] = n > 0.f ? red[1][0] / n : 0.f;
      stats[1] = n > 0.f ? red[2][0] / n : 0.f;
    }
  }
}

// (value, index) a joined with b: the greater value, the smaller index among equals (torch.argmax's first maximum)
ASRX_DEV void maxarg_join(float& mx, int& am, float om, int oa) {
  if (om > mx || (om == mx && oa < am)) { mx = om; am = oa; }
}

// Row-wide (max, first argmax) over WPR waves: xor butterfly inside the wave, the waves' results through LDS, joined
// in wave order by every thread.
template <int WPR>
ASRX_DEV void row_maxarg(float& mx, int& am, float* s_mx, int* s_am, int lane, int w) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float om = __shfl_xor(mx, o, 64);
    const int oa = __shfl_xor(am, o, 64);
    maxarg_join(mx, am, om, oa);
  }
  if (WPR > 1) {
    if (lane == 0) { s_mx[w] = mx; s_am[w] = am; }
    __syncthreads();
    mx = s_mx[0];
    am = s_am[0];
#pragma unroll
    for (int u = 1; u < WPR; ++u) maxarg_join(mx, am, s_mx[u], s_am[u]);
  }
}

// Row-wide sums of a and b, the waves' partial sums added in wave order (s_sum: 2 * WPR floats).
template <int WPR>
ASRX_DEV void row_sum2(float& a, float& b, float* s_sum, int lane, int w) {
  a = wave_sum(a);
  b = wave_sum(b);
  if (WPR > 1) {
    if (lane == 0) { s_sum[2 * w] = a; s_sum[2 * w + 1] = b; }
    __syncthreads();
    a = s_sum[0];
    b = s_sum[1];
#pragma unroll
    for (int u = 1; u < WPR; ++u) { a += s_sum[2 * u]; b += s_sum[2 * u + 1]; }
  }
}

// gradient constants of one row (tc: the target as a column, -1 for one outside [0, V))
struct RowOut { float k, on, u, mx, inv, lse; int64_t t; int tc; };

// the row's scalars (one thread writes them) and its gradient constants
ASRX_DEV RowOut row_finish(const float* x, int64_t r, int64_t rows, int V, const int64_t* tgt, int64_t ignore,
                           float eps, float gscale, float mx, int am, float s, float d, int64_t* argmax,
                           float* ws, bool writer) {
  RowOut o;
  o.lse = mx + __logf(s);
  o.mx = mx;
  o.inv = 1.f / s;
  o.t = tgt[r];
  o.tc = o.t >= 0 && o.t < V ? (int)o.t : -1;
  const bool valid = o.t != ignore;
  const float cnt = ws[3 * rows];
  o.k = valid && cnt > 0.f ? gscale / cnt : 0.f;
  o.on = 1.f - eps;
  o.u = eps / (float)V;
  if (writer) {
    float nll = 0.f, row = 0.f;
    if (valid) {
      // (a target outside [0, V) has no logit: NaN, never an out-of-bounds read)
      const float xt = o.t >= 0 && o.t < V ? x[o.t] : __builtin_nanf("");
      nll = o.lse - xt;
      row = nll;
      if (eps > 0.f) row = (1.f - eps) * nll + eps * (o.lse - (mx + d / (float)V));
    }
    ws[r] = row;
    ws[rows + r] = nll;
    ws[2 * rows + r] = valid && (int64_t)am == o.t ? 1.f : 0.f;
    if (argmax) argmax[r] = am;
  }
  return o;
}

// gradient of column c from e = exp(x - max) (softmax as e / sum: exact at the maximum, where exp(x - lse) would carry
// the rounding of a large lse)
ASRX_DEV float xent_grad(float e, int c, int V, const RowOut& o) {
  if (c >= V || o.k == 0.f) return 0.f;
  return (e * o.inv - (c == o.tc ? o.on : 0.f) - o.u) * o.k;
}

// four gradients to columns c .. c + 3 of a row (8-B bf16 / 16-B fp32 store) or one to column c
ASRX_DEV void store4(void* drow, int gdt, int64_t c, float g0, float g1, float g2, float g3) {
  if (gdt == ASRX_BF16) {
    v2u_t u;
    u.x = pack2bf(g0, g1);
    u.y = pack2bf(g2, g3);
    *(v2u_t*)((bf16_t*)drow + c) = u;
  } else {
    *(f4_t*)((float*)drow + c) = (f4_t){g0, g1, g2, g3};
  }
}
ASRX_DEV void store1(void* drow, int gdt, int64_t c, float g) {
  if (gdt == ASRX_BF16) ((bf16_t*)drow)[c] = f2bf(g);
  else ((float*)drow)[c] = g;
}
ASRX_DEV void* row_ptr(void* dlog, int gdt, int64_t off) {
  return gdt == ASRX_BF16 ? (void*)((bf16_t*)dlog + off) : (void*)((float*)dlog + off);
}

// Register-resident rows: WPR waves per row (4: one row per workgroup; 1: four rows per workgroup, no LDS), NV float4
// (VEC) or 4 NV scalars per thread: rows of up to 256 * WPR * NV columns.
template <int NV, int WPR, bool VEC>
__global__ __launch_bounds__(256) void xent_rows_kernel(const float* __restrict__ logits, int64_t rows, int V,
                                                        int64_t ld, const int64_t* __restrict__ tgt, int64_t ignore,
                                                        float eps, float gscale, int gdt, void* __restrict__ dlog,
                                                        int64_t* __restrict__ argmax, float* __restrict__ ws) {
  constexpr int TPR = 64 * WPR, NE = 4 * NV;
  __shared__ float s_mx[4];
  __shared__ int s_am[4];
  __shared__ float s_sum[8];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int t = WPR == 4 ? (int)threadIdx.x : lane;
  const int w = WPR == 4 ? wave : 0;
  const int64_t r = WPR == 4 ? (int64_t)blockIdx.x : (int64_t)blockIdx.x * 4 + wave;
  if (r >= rows) return;   // (whole waves, and no barrier below, where WPR == 1)
  const float* x = logits + r * ld;
  // element e of this thread is column col(e), ascending in e
  auto col = [&](int e) { return VEC ? ((e >> 2) * TPR + t) * 4 + (e & 3) : e * TPR + t; };
  float v[NE];
  if (VEC) {
#pragma unroll
    for (int j = 0; j < NV; ++j) {
      const int c = (j * TPR + t) * 4;
      if (c + 3 < V) {
        const f4_t q = *(const f4_t*)(x + c);
        v[4 * j] = q[0]; v[4 * j + 1] = q[1]; v[4 * j + 2] = q[2]; v[4 * j + 3] = q[3];
      } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) v[4 * j + k] = c + k < V ? x[c + k] : -INFINITY;
      }
    }
  } else {
#pragma unroll
    for (int e = 0; e < NE; ++e) v[e] = col(e) < V ? x[col(e)] : -INFINITY;
  }
  float mx = -INFINITY;
  int am = 0;
#pragma unroll
  for (int e = 0; e < NE; ++e)
    if (v[e] > mx) { mx = v[e]; am = col(e); }
  row_maxarg<WPR>(mx, am, s_mx, s_am, lane, w);
  float s = 0.f, d = 0.f;
#pragma unroll
  for (int e = 0; e < NE; ++e) {   // (v becomes exp(v - max): the gradient's numerator, computed once)
    const float dv = v[e] - mx;
    d += col(e) < V ? dv : 0.f;
    v[e] = __expf(dv);
    s += v[e];
  }
  row_sum2<WPR>(s, d, s_sum, lane, w);
  const RowOut o = row_finish(x, r, rows, V, tgt, ignore, eps, gscale, mx, am, s, d, argmax, ws, t == 0);
  if (!dlog) return;
  void* drow = row_ptr(dlog, gdt, r * ld);
  if (VEC) {
#pragma unroll
    for (int j = 0; j < NV; ++j) {
      const int c = (j * TPR + t) * 4;
      if (c < ld)
        store4(drow, gdt, c, xent_grad(v[4 * j], c, V, o), xent_grad(v[4 * j + 1], c + 1, V, o),
               xent_grad(v[4 * j + 2], c + 2, V, o), xent_grad(v[4 * j + 3], c + 3, V, o));
    }
  } else {
#pragma unroll
    for (int e = 0; e < NE; ++e)
      if (col(e) < ld) store1(drow, gdt, col(e), xent_grad(v[e], col(e), V, o));
  }
}

// Online softmax state of a set of columns: max m (first at column am), s = sum exp(x - m), d = sum (x - m) over n
// columns.  (-inf columns leave s and n * m sums alone until a finite maximum arrives; d is meaningful for finite
// logits only, which label smoothing assumes.)
struct Online { float m, s, d; int n, am; };

ASRX_DEV void online_raise(Online& a, float m, int am) {   // m > a.m
  if (a.n > 0 && a.m != -INFINITY) {
    const float dm = a.m - m;
    a.s *= __expf(dm);
    a.d += (float)a.n * dm;
  } else {
    a.s = 0.f;
    a.d = 0.f;
  }
  a.m = m;
  a.am = am;
}
ASRX_DEV void online_add(Online& a, float x) {   // x <= a.m
  if (a.m != -INFINITY) {
    a.s += __expf(x - a.m);
    a.d += x - a.m;
  }
  a.n += 1;
}
ASRX_DEV void online_join(Online& a, const Online& b) {
  const float M = fmaxf(a.m, b.m);
  int am = a.am;
  if (b.m > a.m || (b.m == a.m && b.am < a.am)) am = b.am;
  const float sa = a.m == M ? a.s : a.s * __expf(a.m - M), sb = b.m == M ? b.s : b.s * __expf(b.m - M);
  const float da = a.m == M || a.n == 0 ? a.d : a.d + (float)a.n * (a.m - M);
  const float db = b.m == M || b.n == 0 ? b.d : b.d + (float)b.n * (b.m - M);
  a.m = M;
  a.am = am;
  a.s = sa + sb;
  a.d = da + db;
  a.n += b.n;
}

// Streamed rows (ld > 16384): one workgroup per row, two passes over the row.
template <bool VEC>
__global__ __launch_bounds__(256) void xent_stream_kernel(const float* __restrict__ logits, int64_t rows, int V,
                                                          int64_t ld, const int64_t* __restrict__ tgt, int64_t ignore,
                                                          float eps, float gscale, int gdt, void* __restrict__ dlog,
                                                          int64_t* __restrict__ argmax, float* __restrict__ ws) {
  __shared__ Online s_on[4];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int64_t r = blockIdx.x;
  const float* x = logits + r * ld;
  Online a = {-INFINITY, 0.f, 0.f, 0, 0};
  if (VEC) {
#pragma unroll 4
    for (int c = t * 4; c < V; c += 1024) {
      float q[4];
      if (c + 3 < V) {
        const f4_t f = *(const f4_t*)(x + c);
        q[0] = f[0]; q[1] = f[1]; q[2] = f[2]; q[3] = f[3];
      } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) q[k] = c + k < V ? x[c + k] : -INFINITY;
      }
      float vm = a.m;
      int va = a.am;
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (q[k] > vm) { vm = q[k]; va = c + k; }
      if (vm > a.m) online_raise(a, vm, va);
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (c + k < V) online_add(a, q[k]);
    }
  } else {
#pragma unroll 4
    for (int c = t; c < V; c += 256) {
      const float q = x[c];
      if (q > a.m) online_raise(a, q, c);
      online_add(a, q);
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    Online b;
    b.m = __shfl_xor(a.m, o, 64);
    b.s = __shfl_xor(a.s, o, 64);
    b.d = __shfl_xor(a.d, o, 64);
    b.n = __shfl_xor(a.n, o, 64);
    b.am = __shfl_xor(a.am, o, 64);
    online_join(a, b);
  }
  if (lane == 0) s_on[wave] = a;
  __syncthreads();
  a = s_on[0];
#pragma unroll
  for (int u = 1; u < 4; ++u) online_join(a, s_on[u]);
  const RowOut o = row_finish(x, r, rows, V, tgt, ignore, eps, gscale, a.m, a.am, a.s, a.d, argmax, ws, t == 0);
  if (!dlog) return;
  void* drow = row_ptr(dlog, gdt, r * ld);
  if (VEC) {
#pragma unroll 4
    for (int64_t c = t * 4; c < ld; c += 1024) {
      float g[4] = {0.f, 0.f, 0.f, 0.f};
      if (c + 3 < V) {
        const f4_t f = *(const f4_t*)(x + c);
#pragma unroll
        for (int k = 0; k < 4; ++k) g[k] = xent_grad(__expf(f[k] - o.mx), (int)c + k, V, o);
      } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
          if (c + k < V) g[k] = xent_grad(__expf(x[c + k] - o.mx), (int)c + k, V, o);
      }
      store4(drow, gdt, c, g[0], g[1], g[2], g[3]);
    }
  } else {
#pragma unroll 4
    for (int64_t c = t; c < ld; c += 256)
      store1(drow, gdt, c, c < V ? xent_grad(__expf(x[c] - o.mx), (int)c, V, o) : 0.f);
  }
}

}  // namespace

extern "C" int asrx_xent_workspace_elems(int64_t rows) {
  return rows < 0 || rows > ASRX_XENT_MAX_ROWS ? -1 : (int)(3 * rows + 4);
}

extern "C" int asrx_cross_entropy_ls(const float* logits, int64_t rows, int32_t V, int64_t ld, const int64_t* target,
                                     int64_t ignore_index, float label_smoothing, float grad_scale, float* loss,
                                     float* stats, int32_t grad_dtype, void* dlogits, int64_t* argmax, float* ws,
                                     void* stream) {
  if (!logits || !target || !loss || !ws || V <= 0 || ld < V || rows < 0) return ASRX_ERR_ARG;
  if (!(label_smoothing >= 0.f && label_smoothing < 1.f)) return ASRX_ERR_ARG;
  if (grad_dtype != ASRX_BF16 && grad_dtype != ASRX_F32) return ASRX_ERR_ARG;
  if (V > XENT_MAXV || rows > ASRX_XENT_MAX_ROWS) return ASRX_ERR_UNSUPPORTED;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(xent_count_kernel, dim3(1), dim3(256), 0, st, target, rows, ignore_index, ws);
  ASRX_CHECK_LAUNCH();
  if (rows > 0) {
    const bool vec = ld % 4 == 0 && (uintptr_t)logits % 16 == 0 && (uintptr_t)dlogits % 16 == 0;
#define XENT_ARGS \
  logits, rows, V, ld, target, ignore_index, label_smoothing, grad_scale, grad_dtype, dlogits, argmax, ws
#define XENT_ROWS(NV, WPR)                                                                                       \
  do {                                                                                                           \
    const dim3 grid((unsigned)((WPR) == 4 ? rows : (rows + 3) / 4));                                             \
    if (vec) hipLaunchKernelGGL((xent_rows_kernel<NV, WPR, true>), grid, dim3(256), 0, st, XENT_ARGS);           \
    else hipLaunchKernelGGL((xent_rows_kernel<NV, WPR, false>), grid, dim3(256), 0, st, XENT_ARGS);              \
  } while (0)
    if (ld <= 256) XENT_ROWS(1, 1);
    else if (ld <= 512) XENT_ROWS(2, 1);
    else if (ld <= 1024) XENT_ROWS(4, 1);
    else if (ld <= 2048) XENT_ROWS(2, 4);
    else if (ld <= 4096) XENT_ROWS(4, 4);
    else if (ld <= 8192) XENT_ROWS(8, 4);
    else if (ld <= XENT_REG_MAXLD) XENT_ROWS(16, 4);
    else if (vec) hipLaunchKernelGGL((xent_stream_kernel<true>), dim3((unsigned)rows), dim3(256), 0, st, XENT_ARGS);
    else hipLaunchKernelGGL((xent_stream_kernel<false>), dim3((unsigned)rows), dim3(256), 0, st, XENT_ARGS);
#undef XENT_ROWS
#undef XENT_ARGS
    ASRX_CHECK_LAUNCH();
  }
  hipLaunchKernelGGL(xent_final_kernel, dim3(1), dim3(256), 0, st, ws, rows, loss, stats);
  ASRX_CHECK_LAUNCH();
  return ASRX_OK;
}
