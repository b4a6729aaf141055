// Edit distance of token rows of up to 4095 kept tokens.  C-ABI: asrx_edit_distance_long (include/asrx.h).
//
// edit_distance_kernel's wavefront (edit.hip: one wave64 per pair, lane l owning column c0 + l of a 64-column block of
// the reference, the left neighbour by one DPP wave shift, the previous block's last column in LDS) with three changes:
//   - both filtered rows and the column boundary live in DYNAMIC LDS, 2 * 4096 * 8 B + 4096 * 4 B = 80 KiB;
//   - hence one pair (one wave64) per workgroup;
//   - the packed cost is edits << 13 | substitutions: substitutions <= 4095 < 8192, so the minimum of the packed value
//     is still the lexicographic minimum of the pair, and with edits <= 8190 it stays below 2^26.
// From the optimum: edits = packed >> 13, sub = packed & 8191, del = (edits - sub - (len_hyp - len_ref)) / 2,
// ins = del + len_hyp - len_ref.  Integer arithmetic only, no workgroup barrier (one wave), no atomics; every output
// element is written by every call.  On inputs asrx_edit_distance accepts the integers are the same.
#include "common.h"

namespace {

constexpr int EDL_MAXL = ASRX_ED_LONG_MAX_TOKENS;   // tokens of a filtered sequence
constexpr int EDL_SLOTS = EDL_MAXL + 1;
constexpr int EDL_MAXW = 16;                        // hypotheses per group in CROSS mode (asrx_edit_distance's)
constexpr int EDL_SHIFT = 13;
constexpr int EDL_EDIT = 1 << EDL_SHIFT;            // packed cost of an insertion or a deletion; a substitution: + 1
constexpr size_t EDL_LDS = (size_t)EDL_SLOTS * (8 + 8 + 4);

struct EdlFilter {
  int64_t drop[4];
  int64_t stop;   // < 0: none
  int ndrop;
};

// the sequence of row[0 .. len) -> s[0 .. min(count, 4096)); returns the count (> EDL_MAXL: too long, s is incomplete)
ASRX_DEV int edl_load(const int64_t* __restrict__ row, int len, const EdlFilter& f, int64_t* s, int lane) {
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
    if (keep && p <= EDL_MAXL) s[p] = t;
    cnt += __popcll(m);
    if (stopm != 0 || cnt > EDL_MAXL) break;   // (wave-uniform)
  }
  return __builtin_amdgcn_readfirstlane(cnt);
}

__global__ __launch_bounds__(64) void edit_distance_long_kernel(
    const int64_t* __restrict__ hyp, int64_t ld_hyp, int hyp_cols, const int32_t* __restrict__ hyp_len,
    const int64_t* __restrict__ ref, int64_t ld_ref, int ref_cols, const int32_t* __restrict__ ref_len, int mode, int W,
    const int32_t* __restrict__ n_hyp, EdlFilter f, int32_t* __restrict__ dist, int32_t* __restrict__ counts) {
  extern __shared__ int64_t s_edl[];
  int64_t* sh = s_edl;
  int64_t* sr = s_edl + EDL_SLOTS;
  int* bd = (int*)(s_edl + 2 * EDL_SLOTS);
  const int lane = threadIdx.x;
  const int n = blockIdx.x;

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
    const int lh = clamp_len(hyp_len ? hyp_len[hr] : hyp_cols, hyp_cols);
    const int lr = clamp_len(rlen ? rlen[rr] : rcols, rcols);
    m = edl_load(hyp + hr * ld_hyp, lh, f, sh, lane);
    nn = edl_load(rbase + rr * rld, lr, f, sr, lane);
    if (m > EDL_MAXL || nn > EDL_MAXL) code = -2;
  }
  if (code < 0) {   // (wave-uniform; the workgroup is this one wave)
    if (lane == 0) dist[n] = code;
    if (counts && lane < 4) counts[(int64_t)n * 4 + lane] = -1;
    return;
  }

  int packed = EDL_EDIT * (m + nn);   // one side empty: all insertions or all deletions
  if (m > 0 && nn > 0) {
    for (int i = lane; i <= m; i += 64) bd[i] = EDL_EDIT * i;   // column 0: i insertions
    wave_lds_sync();
    const int nblk = (nn + 63) >> 6;
    int v = 0;
    for (int blk = 0; blk < nblk; ++blk) {
      const int c0 = blk << 6, col = c0 + lane;
      const int64_t rt = sr[col < nn ? col : nn - 1];   // (a column past the reference feeds no live column)
      v = EDL_EDIT * (col + 1);                         // row 0: col + 1 deletions
      int lp = EDL_EDIT * col;                          // row 0 of the column to the left
      const int steps = m + (blk == nblk - 1 ? nn - 1 - c0 : 63);
      int64_t ht = sh[0];
      int fill = bd[1];
      for (int s = 0; s < steps; ++s) {
        const int i = s - lane;   // this lane's row (of the hypothesis, 0-based) at this step
        const bool act = (unsigned)i < (unsigned)m;
        const int64_t ht_n = sh[clamp_len(i + 1, m - 1)];   // the next step's operands, read while this one computes
        const int fill_n = bd[s + 2 < m ? s + 2 : m];
        const int left = wave_up1(v, fill);
        const int dg = lp + (ht == rt ? 0 : EDL_EDIT + 1);
        int nv = (v < left ? v : left) + EDL_EDIT;
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
    const int edits = packed >> EDL_SHIFT, sub = packed & (EDL_EDIT - 1);
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

}  // namespace

extern "C" int asrx_edit_distance_long(const int64_t* hyp, int64_t ld_hyp, int32_t hyp_cols, const int32_t* hyp_len,
                                       const int64_t* ref, int64_t ld_ref, int32_t ref_cols, const int32_t* ref_len,
                                       int32_t N, int32_t mode, int32_t W, const int32_t* n_hyp, const int64_t* drop,
                                       int32_t ndrop, int64_t stop_id, int32_t* dist, int32_t* counts, void* stream) {
  if (N <= 0 || !hyp || !dist || hyp_cols <= 0 || ld_hyp < hyp_cols) return ASRX_ERR_ARG;
  if (ndrop < 0 || ndrop > 4 || (ndrop > 0 && !drop)) return ASRX_ERR_ARG;
  if (mode == ASRX_ED_PAIRS || mode == ASRX_ED_GROUP) {
    if (!ref || ref_cols <= 0 || ld_ref < ref_cols) return ASRX_ERR_ARG;
    if (mode == ASRX_ED_GROUP && (W < 1 || N % W != 0)) return ASRX_ERR_ARG;
  } else if (mode == ASRX_ED_CROSS) {
    if (W < 1 || W > EDL_MAXW || N % (W * W) != 0) return ASRX_ERR_ARG;
  } else {
    return ASRX_ERR_ARG;
  }
  EdlFilter f;
  f.ndrop = ndrop;
  f.stop = stop_id < 0 ? -1 : stop_id;
  for (int k = 0; k < 4; ++k) f.drop[k] = k < ndrop ? drop[k] : 0;
  hipLaunchKernelGGL(edit_distance_long_kernel, dim3((unsigned)N), dim3(64), EDL_LDS, (hipStream_t)stream, hyp, ld_hyp,
                     (int)hyp_cols, hyp_len, ref, ld_ref, (int)ref_cols, ref_len, (int)mode,
                     (int)(mode == ASRX_ED_PAIRS ? 1 : W), mode == ASRX_ED_PAIRS ? nullptr : n_hyp, f, dist, counts);
  ASRX_CHECK_LAUNCH();
  return ASRX_OK;
}
