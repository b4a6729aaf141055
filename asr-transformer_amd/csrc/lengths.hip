// Lengths on the device (asrx_length_mask): per-utterance frame counts -> the encoder's row counts and the key-validity
// bytes that mask mode 1 of asrx_attention_fwd / bwd and asrx_softmax_fwd reads (restated in numpy by
// tests/lengths_ref.py).  One launch, no host round trip: a captured training step replays with new lengths.
//
// A workgroup covers LM_RUN columns of one utterance's row; every thread derives the utterance's row count itself (at
// most 8 integer steps), so there is no LDS and no barrier.  One byte per lane, consecutive lanes on consecutive
// columns: valid_bstride need not be aligned.
#include "common.h"

constexpr int LM_RUN = 256;   // columns per workgroup

// the unpadded kernel-3 stride-2 convolution's output length, applied k times, clamped to [0, T]
ASRX_DEV int lm_rows(int n, int k, int T) {
  for (int i = 0; i < k; ++i) n = n < 3 ? 0 : (n - 3) / 2 + 1;
  return clamp_len(n, T);
}

__global__ __launch_bounds__(LM_RUN) void length_mask_kernel(const int32_t* __restrict__ lengths, int B, int T, int k,
                                                             int32_t* __restrict__ enc_lengths,
                                                             uint8_t* __restrict__ valid, int64_t vb, int nchunk) {
  const int tid = threadIdx.x;
  if (!valid) {   // lengths only: one utterance per lane
    const int b = blockIdx.x * LM_RUN + tid;
    if (b < B) enc_lengths[b] = lm_rows(lengths[b], k, T);
    return;
  }
  const int b = blockIdx.x / nchunk, chunk = blockIdx.x % nchunk;
  const int L = lm_rows(lengths[b], k, T);
  if (enc_lengths && chunk == 0 && tid == 0) enc_lengths[b] = L;
  const int t = chunk * LM_RUN + tid;
  if (t < T) valid[(int64_t)b * vb + t] = t < L ? 1 : 0;
}

extern "C" int asrx_length_mask(const int32_t* lengths, int32_t B, int32_t T, int32_t subsample, int32_t* enc_lengths,
                                uint8_t* valid, int64_t valid_bstride, void* stream) {
  if (!lengths || B < 0 || T <= 0 || subsample < 0 || subsample > 8) return ASRX_ERR_ARG;
  if (!enc_lengths && !valid) return ASRX_ERR_ARG;
  if (valid_bstride < T) return ASRX_ERR_ARG;
  if (B == 0) return ASRX_OK;
  const int nchunk = cdiv(T, LM_RUN);
  const int64_t blocks = valid ? (int64_t)B * nchunk : (int64_t)cdiv(B, LM_RUN);
  if (blocks > 0x7fffffffLL) return ASRX_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(length_mask_kernel, dim3((unsigned)blocks), dim3(LM_RUN), 0, (hipStream_t)stream, lengths, B, T,
                     subsample, enc_lengths, valid, valid_bstride, nchunk);
  ASRX_CHECK_LAUNCH();
  return ASRX_OK;
}
