"""The whole input pipeline on the device: waveform -> LogMel -> CMVN -> SpecAugment ->
Trainer.step(input_lengths=), the frame lengths produced once and accepted everywhere; the global CMVN route
(accumulate, finalize, state_dict, fused into LogMel); MelSpectrogram.

Bound of the LogMel -> utterance-CMVN features against the restatement.  With lb the log bound of
tests/test_gpu_fbank_kernels.py (the error dv the log-mel values may carry), a row's output (v - mean) * istd moves by
(dv - mean(dv)) * istd - ref * dsigma / sigma with |dsigma| <= max|dv - mean(dv)|, so
|out - ref| <= (lb[t] + mean(lb)) * istd + |ref| * (max(lb) + mean(lb)) * istd + 5e-5 * (1 + |ref|),
the last term asrx_cmvn's own bound."""
import numpy as np
import pytest
import torch

import fbank_ref as R
from tests import specaug_ref

pytestmark = pytest.mark.gpu
dev = "cuda"
N_FFT, HOP, MELS = 400, 160, 80
LENGTHS = [16000, 9000]
AUG = dict(freq_masks=2, freq_width=27, time_masks=2, time_width=20, time_ratio=1.0, time_warp=0)
SEED = 5


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _np(t):
    return t.detach().cpu().double().numpy()


def _log_bound(e_ref, eps=1e-6):
    return 4e-5 * e_ref.max() / (e_ref + eps) + 1e-6


@pytest.fixture(scope="module")
def pipeline():
    """(waveform numpy (2, 1, 16000), features (2, 1, 80, 98) on the device, frame_lengths, the restatement's features)"""
    import asrx
    x = R.waveform((2, 1, 16000), seed=21)
    feats, fl = asrx.LogMel(n_fft=N_FFT, hop_length=HOP, n_mels=MELS)(torch.from_numpy(x).to(dev), lengths=LENGTHS)
    assert tuple(feats.shape) == (2, 1, MELS, 98) and fl.dtype == torch.int32 and fl.tolist() == [98, 54]
    feats = asrx.CMVN(MELS, mode="utterance")(feats, lengths=fl)
    assert tuple(feats.shape) == (2, 1, MELS, 98)
    fb = R.melscale_fbanks(N_FFT // 2 + 1, 0.0, 8000.0, MELS, 16000)
    v, e, rfl = R.logmel(x[:, 0], fb, N_FFT, HOP, lengths=LENGTHS)
    assert rfl.tolist() == [98, 54]
    ref = R.cmvn_utterance(v, rfl)
    lb = _log_bound(e)
    bound = np.zeros_like(ref)
    for b, L in enumerate(rfl):
        row, lbr = v[b, :, :L], lb[b, :, :L]
        istd = 1.0 / np.maximum(row.std(axis=1, keepdims=True), 1e-5)
        mean_lb, max_lb = lbr.mean(axis=1, keepdims=True), lbr.max(axis=1, keepdims=True)
        r = np.abs(ref[b, :, :L])
        bound[b, :, :L] = (lbr + mean_lb) * istd + r * (max_lb + mean_lb) * istd + 5e-5 * (1.0 + r)
    return x, feats, fl, ref, bound


def test_pipeline_features_match_the_restatement(pipeline):
    _, feats, fl, ref, bound = pipeline
    o = _np(feats[:, 0])
    assert (o[1, :, 54:] == 0.0).all()
    err = np.abs(o - ref)
    print(f"LogMel -> CMVN: max err {err.max():.3g}, max err / bound {(err / np.maximum(bound, 1e-30))[:, :, :54].max():.3g}")
    assert (err <= bound).all()


@pytest.mark.parametrize("graph", [False, True])
def test_waveform_to_training_step(pipeline, graph):
    import asrx
    from asrx.train import Trainer
    _, feats, fl, _, _ = pipeline
    aug = asrx.SpecAugment(seed=SEED, **AUG).train()
    by_hand = aug(feats, lengths=fl, step=3)
    want3, mag, _ = specaug_ref.specaug(_np(feats), fl.tolist(), seed=SEED, step=3, **AUG)
    assert not mag.any()
    want3 = torch.from_numpy(want3.astype(np.float32))
    assert torch.equal(by_hand.cpu(), want3) and not torch.equal(want3, feats.cpu())
    torch.manual_seed(3)
    m = asrx.Transformer(250, MELS, 128, 16, 98, 1, 1, 4, 512, dropout=0.0, precision="bf16", ctc=True).to(dev).train()
    g = torch.Generator().manual_seed(4)
    text = torch.randint(5, 250, (2, 9), generator=g)
    text[:, 0] = 1
    text, mask = text.to(dev), torch.ones(2, 9, device=dev)
    tr = Trainer(m, lr=1e-3, graph=graph, ctc_weight=0.3, spec_augment=aug)
    keep = feats.clone()
    losses = [float(tr.step(feats, text, mask, input_lengths=fl)) for _ in range(3)]
    torch.cuda.synchronize()
    assert all(np.isfinite(losses)), losses
    assert torch.equal(feats, keep)
    assert (tr._cap is not None) == graph
    if graph:   # what the trainer saw at step 3: the reference's augmentation of these features, bit for bit
        assert torch.equal(tr._cap[1][0].cpu(), want3)
    # the same frame lengths, subsampled, for the CTC decoders
    tok, n = m.eval().ctc_greedy(feats, input_lengths=asrx.subsampled(fl))
    assert asrx.subsampled(fl).tolist() == [asrx.subsampled(98), asrx.subsampled(54)]
    assert tok.shape[0] == 2 and n.dtype == torch.int32 and int(n[1]) <= asrx.subsampled(54)


def test_global_cmvn_route(pipeline):
    """accumulate over two batches, finalize, a state_dict round trip, and LogMel(cmvn=) against LogMel() followed by
    the standalone global CMVN (held to the fused-CMVN bound: the two round differently)."""
    import asrx
    x = pipeline[0]
    xg = torch.from_numpy(x).to(dev)
    plain = asrx.LogMel(n_fft=N_FFT, hop_length=HOP, n_mels=MELS)
    v1, fl1 = plain(xg, lengths=LENGTHS)
    x2 = R.waveform((3, 1, 7001), seed=22)
    v2, fl2 = plain(torch.from_numpy(x2).to(dev), lengths=[7001, 399, 560])
    cm = asrx.CMVN(MELS, mode="global").to(dev)
    with pytest.raises(RuntimeError):
        asrx.LogMel(n_fft=N_FFT, hop_length=HOP, n_mels=MELS, cmvn=cm)(xg)      # not finalised
    cm.accumulate(v1, fl1).accumulate(v2, fl2)
    cm.finalize()
    s, q, n = R.feature_sums([(_np(v1[:, 0]), fl1.tolist()), (_np(v2[:, 0]), fl2.tolist())])
    assert int(cm.count) == n == 98 + 54 + 42 + 0 + 2
    mean, istd = R.finalize(s, q, n)
    assert np.abs(_np(cm.mean) - mean).max() <= 1e-6 and (np.abs(_np(cm.istd) - istd) <= 1e-6 * istd).all()
    fresh = asrx.CMVN(MELS, mode="global")
    fresh.load_state_dict(cm.state_dict())
    fresh = fresh.to(dev)
    assert torch.equal(fresh.mean, cm.mean) and torch.equal(fresh.istd, cm.istd)
    fused, flf = asrx.LogMel(n_fft=N_FFT, hop_length=HOP, n_mels=MELS, cmvn=fresh)(xg, lengths=LENGTHS)
    two_step = fresh(v1, lengths=fl1)
    assert flf.tolist() == fl1.tolist() == [98, 54]
    fb = R.melscale_fbanks(N_FFT // 2 + 1, 0.0, 8000.0, MELS, 16000)
    ref, e, _ = R.logmel(x[:, 0], fb, N_FFT, HOP, mean=_np(cm.mean), istd=_np(cm.istd), lengths=LENGTHS)
    bound = _log_bound(e) * _np(cm.istd)[None, :, None] + 1e-6 * (1.0 + np.abs(ref))
    for got in (fused, two_step):
        o = _np(got[:, 0])
        assert (o[1, :, 54:] == 0.0).all()
        assert (np.abs(o - ref) <= bound).all()
    assert (np.abs(_np(fused) - _np(two_step))[:, 0] <= 2.0 * bound).all()


def test_melspectrogram_is_logmel_without_the_log(pipeline):
    from asrx.features import LogMel, MelSpectrogram
    xg = torch.from_numpy(pipeline[0]).to(dev)
    a = MelSpectrogram(n_fft=N_FFT, hop_length=HOP)(xg)
    b = LogMel(n_fft=N_FFT, hop_length=HOP, n_mels=128, log=None)(xg)
    assert tuple(a.shape) == (2, 1, 128, 98) and torch.equal(a, b)
