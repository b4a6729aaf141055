"""Trainer(..., spec_augment=SpecAugment(...)): step n trains on the augmentation of step n of its spectrogram, in
eager and in replayed steps alike.  The standard is tests/test_gpu_graph.py's: with dropout 0 every kernel is
deterministic, so a trainer that augments on the device and a plain trainer fed the reference-augmented spectrograms
(tests/specaug_ref.py; masks only, so the reference is exact) must agree bit for bit.  c1, bf16, dropout 0."""
import numpy as np
import pytest
import torch

from oracle.ref_model import CONFIGS, det_params, synthetic_batch
from tests import specaug_ref as R

pytestmark = pytest.mark.gpu
dev = "cuda"
AUG = dict(freq_masks=2, freq_width=27, time_masks=2, time_width=20, time_ratio=1.0, time_warp=0)
SEED = 7


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def build(ctc=False):
    import asrx
    cfg = CONFIGS["c1"]["cfg"]
    torch.manual_seed(11)            # the CTC head's initial values (every other parameter is overwritten below)
    m = asrx.Transformer(cfg.vocab_size, cfg.input_dim, cfg.d_model, cfg.dec_len, cfg.enc_len, cfg.n_enc, cfg.n_dec,
                         cfg.n_heads, cfg.ff_dim, dropout=0.0, precision="bf16", ctc=ctc)
    sd = m.state_dict()
    sd.update(det_params(cfg, 0))
    m.load_state_dict(sd)
    return m.to(dev).train(), cfg


def batches(n):
    spec = CONFIGS["c1"]
    return [synthetic_batch(spec["cfg"], spec["batch"], spec["frames"], spec["text_len"] + 1, seed=100 + i)
            for i in range(n)]


def ref_augmented(s, step, lengths=None):
    out, mag, _ = R.specaug(s.numpy(), lengths, seed=SEED, step=step, **AUG)
    assert not mag.any()
    got = torch.from_numpy(out.astype(np.float32))
    assert not torch.equal(got, s)
    return got


def run_pair(graph, lengths=None, ctc=False):
    """(losses, parameters) of six steps: the augmenting trainer on the raw batches, the plain trainer on the
    reference-augmented ones."""
    import asrx
    from asrx.train import Trainer
    data = batches(6)
    kw = dict(ctc_weight=0.3) if ctc else {}
    lens = None if lengths is None else torch.tensor(lengths, dtype=torch.int32, device=dev)
    out = []
    for augment in (True, False):
        m, cfg = build(ctc)
        tr = Trainer(m, lr=1e-3, graph=graph, spec_augment=asrx.SpecAugment(seed=SEED, **AUG) if augment else None, **kw)
        losses = []
        for n, (s, t, k) in enumerate(data, start=1):
            if augment:
                sd = s.to(dev)
                keep = sd.clone()
                losses.append(float(tr.step(sd, t.to(dev), k.to(dev), input_lengths=lens)))
                assert torch.equal(sd, keep), "the caller's spectrogram was written"
            else:
                losses.append(float(tr.step(ref_augmented(s, n, lengths).to(dev), t.to(dev), k.to(dev))))
        torch.cuda.synchronize()
        assert (tr._cap is not None) == graph
        assert tr.step_count == 6
        out.append((losses, tr.store.flat.clone()))
    return out


@pytest.mark.parametrize("graph", [False, True])
def test_augmenting_trainer_equals_plain_trainer_on_reference_inputs(graph):
    (la, pa), (lb, pb) = run_pair(graph)
    assert la == lb
    assert torch.equal(pa, pb)


@pytest.mark.parametrize("graph", [False, True])
def test_with_input_lengths(graph):
    (la, pa), (lb, pb) = run_pair(graph, lengths=[100, 73, 40, 9])
    assert la == lb
    assert torch.equal(pa, pb)


@pytest.mark.parametrize("graph", [False, True])
def test_with_the_hybrid_ctc_objective(graph):
    (la, pa), (lb, pb) = run_pair(graph, ctc=True)
    assert la == lb
    assert torch.equal(pa, pb)


def test_replays_draw_fresh_masks_and_leave_the_input_alone():
    """The same batch every step at lr = 0: each replay's loss differs (seed 7: the reference's plans of steps 3-6
    differ pairwise), and the caller's spectrogram keeps its bits."""
    import asrx
    from asrx.train import Trainer
    s, t, k = batches(1)[0]
    plans = [R.plan(s.shape[0], s.shape[2], s.shape[3], seed=SEED, step=n, freq_masks=2, freq_width=27, time_masks=2,
                    time_width=20).tobytes() for n in range(3, 7)]
    assert len(set(plans)) == 4
    m, cfg = build()
    tr = Trainer(m, lr=0.0, graph=True, spec_augment=asrx.SpecAugment(seed=SEED, **AUG))
    sd, td, kd = s.to(dev), t.to(dev), k.to(dev)
    losses = [float(tr.step(sd, td, kd)) for _ in range(6)]
    torch.cuda.synchronize()
    assert tr._cap is not None
    replays = losses[2:]
    assert len(set(replays)) == len(replays), losses
    assert torch.equal(sd.cpu(), s)
    # the captured input buffer holds the augmentation of the last step
    assert torch.equal(tr._cap[1][0].cpu(), ref_augmented(s, 6))


def test_captured_buffer_as_input_is_refused():
    import asrx
    from asrx.train import Trainer
    s, t, k = batches(1)[0]
    m, cfg = build()
    tr = Trainer(m, lr=0.0, graph=True, spec_augment=asrx.SpecAugment(seed=SEED, **AUG))
    sd, td, kd = s.to(dev), t.to(dev), k.to(dev)
    for _ in range(3):
        tr.step(sd, td, kd)
    assert tr._cap is not None
    before = tr.step_count
    with pytest.raises(ValueError):
        tr.step(tr._cap[1][0], td, kd)
    assert tr.step_count == before
    torch.cuda.synchronize()
