// Edit distance of token rows on the device, and minimum-Bayes-risk ranking of an n-best list from its pairwise
// distances.  C-ABI: asrx_edit_distance, asrx_mbr_rank (include/asrx.h).
//
//   1. edit_distance_kernel   one wave64 per (hypothesis, reference) pair, four pairs per workgroup, two phases.
//      load       each row is filtered into LDS, 64 entries per round: the entries before the row's length and before
//                 the first stop id that are none of the drop ids, left-packed by a __ballot and a popcount prefix (the
//                 greedy decoder's idiom).  Tokens are only ever compared, never used as an index.  A row that keeps
//                 more than 255 tokens makes its pairs unsupported (dist -2).
//      wavefront  the Levenshtein recursion on packed costs (edits * 512 + substitutions: its minimum is the
//                 lexicographic minimum of the pair, as substitutions <= 255 < 512), over 64-column blocks of the
//                 reference.  Lane l owns column c0 + l and keeps its reference token and its cell in registers; at
//                 step s it computes row s - l from its own previous value (up), lane l - 1's previous value (left,
//                 one DPP wave shift) and the value that shift delivered one step earlier (diagonal).  Lane 0's left
//                 neighbour is the previous block's last column, len_hyp + 1 packed ints that stay in LDS and that
//                 lane 63 overwrites in place 63 steps after lane 0 read them.  The hypothesis token and the boundary
//                 value of the next step are read from LDS while the current step is computed.  ceil(len_ref / 64) *
//                 (len_hyp + 63) steps at most (the last block stops at its last live column), no barrier, no global
//                 traffic after the load.
//      From the optimum: edits = packed >> 9, sub = packed & 511, and as ins - del = len_hyp - len_ref,
//      del = (edits - sub - (len_hyp - len_ref)) / 2, ins = del + len_hyp - len_ref.
//   2. mbr_rank_kernel        one wave per sample, lane i holding hypothesis i: the posterior over the live slots
//                 (max-subtracted), the risks summed in slot order, and the rank by counting (asrx_rescore_rank's
//                 total order).
// Integer arithmetic only in 1: the same inputs give the same bits on any device.  No atomics; every output element
// is written by every call.
#include "common.h"

namespace {

constexpr int ED_MAXL = 255;     // tokens of a filtered sequence
constexpr int ED_WAVES = 4;      // pairs per workgroup
constexpr int ED_MAXW = 16;      // hypotheses per group in CROSS mode and in asrx_mbr_rank
constexpr int ED_EDIT = 512;     // packed cost of an insertion or a deletion; a substitution costs ED_EDIT + 1

struct EdFilter {
  int64_t drop[4];
  int64_t stop;   // < 0: none
  int ndrop;
};

// the sequence of row[0 .. len) -> s[0 .. min(count, 256)); returns the count (> ED_MAXL: too long, s is incomplete)
ASRX_DEV int ed_load(const int64_t* __restrict__ row, int len, const EdFilter& f, int64_t* s, int lane) {
  int cnt = 0;
  for (int c0 = 0; c0 < len; c0 += 64) {
    const int c = c0 + lane;
    const bool in = c < len;
    const int64_t t = in ? row[c] : 0;
    const uint64_t stopm = __ballot(in && f.stop >= 0 && t == f.stop);
    bool keep = in && (stopm == 0 || lane < __ffsll((unsigned long long)stopm) - 1);
#pragma unroll
    for (int k = 0; k < 4; ++k) keep = keep && !(k < f.ndrop && t == f.drop[k]);
    const uint64_t m = __ballot(keep);
    const int p = cnt + __popcll(m & ((1ull << lane) - 1));
    if (keep && p <= ED_MAXL) s[p] = t;
    cnt += __popcll(m);
    if (stopm != 0 || cnt > ED_MAXL) break;   // (wave-uniform)
  }
  return __builtin_amdgcn_readfirstlane(cnt);   // (uniform already: the loops over it below run on the scalar unit)
}

__global__ __launch_bounds__(64 * ED_WAVES) void edit_distance_kernel(
    const int64_t* __restrict__ hyp, int64_t ld_hyp, int hyp_cols, const int32_t* __restrict__ hyp_len,
    const int64_t* __restrict__ ref, int64_t ld_ref, int ref_cols, const int32_t* __restrict__ ref_len, int N, int mode,
    int W, const int32_t* __restrict__ n_hyp, EdFilter f, int32_t* __restrict__ dist, int32_t* __restrict__ counts) {
  __shared__ int64_t s_h[ED_WAVES][ED_MAXL + 1], s_r[ED_WAVES][ED_MAXL + 1];
  __shared__ int s_b[ED_WAVES][ED_MAXL + 1];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int n = blockIdx.x * ED_WAVES + wv;
  if (n >= N) return;   // (no workgroup barrier below: a wave may leave alone)
  int64_t* sh = s_h[wv];
  int64_t* sr = s_r[wv];
  int* bd = s_b[wv];

  // the pair's two rows
  int64_t hr = n, rr = n;
  bool absent = false;
  const int64_t* rbase = ref;
  int64_t rld = ld_ref;
  int rcols = ref_cols;
  const int32_t* rlen = ref_len;
  if (mode == ASRX_ED_GROUP) {
    rr = n / W;
    absent = n_hyp && (n % W) >= n_hyp[rr];
  } else if (mode == ASRX_ED_CROSS) {
    const int g = n / (W * W), i = (n / W) % W, j = n % W;
    hr = (int64_t)g * W + i;
    rr = (int64_t)g * W + j;
    rbase = hyp;
    rld = ld_hyp;
    rcols = hyp_cols;
    rlen = hyp_len;
    if (n_hyp) {
      const int nh = n_hyp[g];
      absent = i >= nh || j >= nh;
    }
  }
  int code = 0, m = 0, nn = 0;
  if (absent) {
    code = -1;
  } else {
    int lh = hyp_len ? hyp_len[hr] : hyp_cols;
    lh = lh < 0 ? 0 : (lh > hyp_cols ? hyp_cols : lh);
    int lr = rlen ? rlen[rr] : rcols;
    lr = lr < 0 ? 0 : (lr > rcols ? rcols : lr);   // (both written out: through clamp_len this kernel's code moves)
    m = ed_load(hyp + hr * ld_hyp, lh, f, sh, lane);
    nn = ed_load(rbase + rr * rld, lr, f, sr, lane);
    if (m > ED_MAXL || nn > ED_MAXL) code = -2;
  }
  if (code < 0) {   // (wave-uniform)
    if (lane == 0) dist[n] = code;
    if (counts && lane < 4) counts[(int64_t)n * 4 + lane] = -1;
    return;
  }

  int packed = ED_EDIT * (m + nn);   // one side empty: all insertions or all deletions
  if (m > 0 && nn > 0) {
    for (int i = lane; i <= m; i += 64) bd[i] = ED_EDIT * i;   // column 0: i insertions
    wave_lds_sync();
    const int nblk = (nn + 63) >> 6;
    int v = 0;
    for (int blk = 0; blk < nblk; ++blk) {
      const int c0 = blk << 6, col = c0 + lane;
      const int64_t rt = sr[col < nn ? col : nn - 1];   // (a column past the reference feeds no live column)
      v = ED_EDIT * (col + 1);                          // row 0: col + 1 deletions
      int lp = ED_EDIT * col;                           // row 0 of the column to the left
      const int steps = m + (blk == nblk - 1 ? nn - 1 - c0 : 63);
      int64_t ht = sh[0];
      int fill = bd[1];
      for (int s = 0; s < steps; ++s) {
        const int i = s - lane;   // this lane's row (of the hypothesis, 0-based) at this step
        const bool act = (unsigned)i < (unsigned)m;
        const int64_t ht_n = sh[clamp_len(i + 1, m - 1)];   // the next step's operands, read while this one computes
        const int fill_n = bd[s + 2 < m ? s + 2 : m];
        const int left = wave_up1(v, fill);
        const int dg = lp + (ht == rt ? 0 : ED_EDIT + 1);
        int nv = (v < left ? v : left) + ED_EDIT;
        nv = nv < dg ? nv : dg;
        v = act ? nv : v;
        lp = left;
        if (lane == 63 && act) bd[i + 1] = v;   // the next block's left boundary (read there 63 steps earlier)
        ht = ht_n;
        fill = fill_n;
      }
      wave_lds_sync();
    }
    packed = __shfl(v, (nn - 1) & 63, 64);
  }
  if (lane == 0) {
    const int edits = packed >> 9, sub = packed & 511;
    dist[n] = edits;
    if (counts) {
      const int del = (edits - sub - (m - nn)) / 2;
      int32_t* c = counts + (int64_t)n * 4;
      c[0] = sub;
      c[1] = del;
      c[2] = del + (m - nn);
      c[3] = nn;
    }
  }
}

// a ranks before b: smaller risk, then lower slot
ASRX_DEV bool ed_before(float ar, int ai, float br, int bi) { return ar < br || (ar == br && ai < bi); }

__global__ __launch_bounds__(64) void mbr_rank_kernel(const int32_t* __restrict__ dist, const float* __restrict__ score,
                                                      const int32_t* __restrict__ n_hyp, int W, float scale,
                                                      float* __restrict__ risk, int32_t* __restrict__ order) {
  const int b = blockIdx.x, lane = threadIdx.x;
  const int32_t* D = dist + (int64_t)b * W * W;
  const int nh = n_hyp ? n_hyp[b] : W;
  float s = -INFINITY;
  bool live = false;
  if (lane < W) {
    s = score[(int64_t)b * W + lane];
    // (a slot whose own distance is negative, absent or too long for asrx_edit_distance, is dead as well)
    live = lane < nh && s > -INFINITY && s < INFINITY && D[lane * W + lane] >= 0;
  }
  const float mx = wave_max(live ? s : -INFINITY);
  float e = 0.f;
  if (live) {
    const float d = s - mx;
    e = d == 0.f ? 1.f : expf(scale * d);   // (the best slot weighs 1 whatever the scale is)
  }
  float sum = 0.f;
  for (int j = 0; j < W; ++j) sum += __shfl(e, j, 64);   // ascending j; a dead slot adds an exact 0
  const float p = live ? e / sum : 0.f;
  float r = 0.f;
  for (int j = 0; j < W; ++j) {
    const float pj = __shfl(p, j, 64);
    const int lj = __shfl((int)live, j, 64);
    if (lj && live) r = __builtin_fmaf(pj, (float)D[lane * W + j], r);
  }
  if (!live) r = INFINITY;
  int rank = 0;
  for (int j = 0; j < W; ++j) {
    const float o = __shfl(r, j, 64);
    rank += ed_before(o, j, r, lane) ? 1 : 0;
  }
  if (lane < W) {
    risk[(int64_t)b * W + lane] = r;
    order[(int64_t)b * W + rank] = lane;
  }
}

}  // namespace

extern "C" int asrx_edit_distance(const int64_t* hyp, int64_t ld_hyp, int32_t hyp_cols, const int32_t* hyp_len,
                                  const int64_t* ref, int64_t ld_ref, int32_t ref_cols, const int32_t* ref_len,
                                  int32_t N, int32_t mode, int32_t W, const int32_t* n_hyp, const int64_t* drop,
                                  int32_t ndrop, int64_t stop_id, int32_t* dist, int32_t* counts, void* stream) {
  if (N <= 0 || !hyp || !dist || hyp_cols <= 0 || ld_hyp < hyp_cols) return ASRX_ERR_ARG;
  if (ndrop < 0 || ndrop > 4 || (ndrop > 0 && !drop)) return ASRX_ERR_ARG;
  if (mode == ASRX_ED_PAIRS || mode == ASRX_ED_GROUP) {
    if (!ref || ref_cols <= 0 || ld_ref < ref_cols) return ASRX_ERR_ARG;
    if (mode == ASRX_ED_GROUP && (W < 1 || N % W != 0)) return ASRX_ERR_ARG;
  } else if (mode == ASRX_ED_CROSS) {
    if (W < 1 || W > ED_MAXW || N % (W * W) != 0) return ASRX_ERR_ARG;
  } else {
    return ASRX_ERR_ARG;
  }
  EdFilter f;
  f.ndrop = ndrop;
  f.stop = stop_id < 0 ? -1 : stop_id;
  for (int k = 0; k < 4; ++k) f.drop[k] = k < ndrop ? drop[k] : 0;
  hipLaunchKernelGGL(edit_distance_kernel, dim3((unsigned)((N + ED_WAVES - 1) / ED_WAVES)), dim3(64 * ED_WAVES), 0,
                     (hipStream_t)stream, hyp, ld_hyp, (int)hyp_cols, hyp_len, ref, ld_ref, (int)ref_cols, ref_len,
                     (int)N, (int)mode, (int)(mode == ASRX_ED_PAIRS ? 1 : W), mode == ASRX_ED_PAIRS ? nullptr : n_hyp,
                     f, dist, counts);
  ASRX_CHECK_LAUNCH();
  return ASRX_OK;
}

extern "C" int asrx_mbr_rank(const int32_t* dist, const float* score, const int32_t* n_hyp, int32_t B, int32_t W,
                             float scale, float* risk, int32_t* order, void* stream) {
  if (!dist || !score || !risk || !order || B <= 0 || W < 1 || W > ED_MAXW) return ASRX_ERR_ARG;
  if (!(scale >= 0.f)) return ASRX_ERR_ARG;   // (negative or NaN)
  hipLaunchKernelGGL(mbr_rank_kernel, dim3((unsigned)B), dim3(64), 0, (hipStream_t)stream, dist, score, n_hyp, (int)W,
                     scale, risk, order);
  ASRX_CHECK_LAUNCH();
  return ASRX_OK;
}
