"""Host-side rules of asrx.decode, no GPU and no native library: how a beam step fuses its score sources
(fusion_rule) and that every argument check fails alike, and before any device work, at the Transformer entry and at
the Decoder entry."""
import types

import pytest
import torch

from oracle.ref_model import CONFIGS


class Source:
    """Stands in for kernels.CtcPrefix / kernels.NgramState: records what is called on it."""

    def __init__(self, name, log):
        self.name, self.log = name, log

    def score(self, *args):
        self.log.append((self.name, "score") + args)

    def advance(self, *args):
        self.log.append((self.name, "advance") + args)


@pytest.mark.parametrize("lam", [0.0, 0.3])
@pytest.mark.parametrize("beta", [0.0, 0.5])
def test_fusion_rule_rows_and_advance_order(lam, beta):
    """The four rows of the rule: the calls that fill the extra matrix, the selecting entry point with its matrix and
    (att_weight, extra_weight), and the advance order CTC, then LM."""
    from asrx import kernels as K
    from asrx.decode import fusion_rule
    log, eos, bonus = [], 22, 0.2
    prefix = Source("ctc", log) if lam > 0 else None
    ngram = Source("lm", log) if beta > 0 else None
    scores, select, joint, sources = fusion_rule(lam, beta, bonus, eos, prefix, ngram, "delta", "extra")
    for fn, args in scores:
        fn(*args)
    for src in sources:
        src.advance(eos, "parent", "tok", "fin")
    adv = (eos, "parent", "tok", "fin")
    if lam == 0 and beta == 0:
        assert select is K.beam_step and joint == () and log == []
        return
    assert select is K.beam_step_joint
    if beta == 0:           # CTC alone: delta unscaled, weighted in the selection
        assert joint == ("delta", 1.0 - lam, lam)
        assert log == [("ctc", "score", eos, "delta"), ("ctc", "advance") + adv]
    elif lam == 0:          # LM alone: att_weight exactly 1
        assert joint == ("extra", 1.0, 1.0)
        assert log == [("lm", "score", "extra", None, 0.0, beta, bonus), ("lm", "advance") + adv]
    else:                   # both: lam folded into extra by the LM's launch
        assert joint == ("extra", 1.0 - lam, 1.0)
        assert log == [("ctc", "score", eos, "delta"), ("lm", "score", "extra", "delta", lam, beta, bonus),
                       ("ctc", "advance") + adv, ("lm", "advance") + adv]


def cpu_model():
    import asrx
    cfg = CONFIGS["micro"]["cfg"]
    return cfg, asrx.Transformer(cfg.vocab_size, cfg.input_dim, cfg.d_model, cfg.dec_len, cfg.enc_len, cfg.n_enc,
                                 cfg.n_dec, cfg.n_heads, cfg.ff_dim, ctc=True).eval()


def raised(fn):
    with pytest.raises((ValueError, RuntimeError)) as e:
        fn()
    return type(e.value), str(e.value)


BAD_LM = types.SimpleNamespace(vocab_size=3)
SEARCH = [
    (dict(ctc_weight=1.5), "ctc_weight 1.5 outside [0, 1]"),
    (dict(lm=BAD_LM, lm_weight=-1.0), "lm_weight -1.0 must be a finite number >= 0"),
    (dict(lm=BAD_LM, lm_weight=0.5, token_bonus=float("inf")), "token_bonus inf must be finite"),
    (dict(lm=BAD_LM, lm_weight=0.5), "the LM's vocabulary (3) is not the classifier's"),
    (dict(lm="lm", lm_weight=0.5, prompt=3), "lm_weight > 0 takes a one-token prompt, got L0 = 3"),
    (dict(ctc_weight=0.3, prompt=3), "ctc_weight > 0 takes a one-token prompt, got L0 = 3"),
    (dict(beam=17), "beam must be in 1..16, got 17"),
    (dict(beam=2, nbest=3), "nbest must be in 1..beam, got 3"),
]


@pytest.mark.parametrize("kw,text", SEARCH, ids=[t for _, t in SEARCH])
def test_search_checks_fail_alike_and_before_device_work(kw, text):
    """The model is on the CPU and the decoder entry gets no encoder output at all: anything but the argument's
    ValueError would be another error, from the first device object touched."""
    cfg, m = cpu_model()
    kw = dict(kw)
    prompt = torch.ones(2, kw.pop("prompt", 1), dtype=torch.int64)
    if kw.get("lm") == "lm":
        kw["lm"] = types.SimpleNamespace(vocab_size=cfg.vocab_size)
    front = raised(lambda: m.beam_search(torch.zeros(2, 1, cfg.input_dim, 60), prompt, **kw))
    ctc = (None, 1, 0, None) if "ctc_weight" in kw else None
    inner = raised(lambda: m.decoder.beam_search(prompt, None, ctc=ctc, **kw))
    assert front == inner and front[0] is ValueError and text in front[1]


RESCORE = [
    (dict(ctc_weight=-1.0), "ctc_weight -1.0 must be >= 0"),
    (dict(lm=BAD_LM, lm_weight=float("nan")), "lm_weight nan must be a finite number >= 0"),
    (dict(mbr_scale=-2.0), "mbr_scale -2.0 must be >= 0"),
    (dict(beam=0), "beam must be in 1..16, got 0"),
    (dict(beam=4, nbest=5), "nbest must be in 1..beam, got 5"),
]


@pytest.mark.parametrize("kw,text", RESCORE, ids=[t for _, t in RESCORE])
def test_rescore_checks_fail_alike_and_before_device_work(kw, text):
    cfg, m = cpu_model()
    front = raised(lambda: m.rescore(torch.zeros(2, 1, cfg.input_dim, 60), **kw))
    inner = raised(lambda: m.decoder.rescore(None, (None, 1, 0, None), **kw))
    assert front == inner and front[0] is ValueError and text in front[1]


def test_missing_ctc_input_is_a_runtime_error_at_both_entries():
    """Each entry names what it lacks (the head, the head's logits), as a RuntimeError, after the value checks."""
    import asrx
    cfg = CONFIGS["micro"]["cfg"]
    m = asrx.Transformer(cfg.vocab_size, cfg.input_dim, cfg.d_model, cfg.dec_len, cfg.enc_len, cfg.n_enc, cfg.n_dec,
                         cfg.n_heads, cfg.ff_dim).eval()
    s, bos = torch.zeros(2, 1, cfg.input_dim, 60), torch.ones(2, 1, dtype=torch.int64)
    assert raised(lambda: m.beam_search(s, ctc_weight=0.3)) == (
        RuntimeError, "asrx: ctc_weight > 0 needs a model with a CTC head (Transformer(..., ctc=True))")
    assert raised(lambda: m.decoder.beam_search(bos, None, ctc_weight=0.3)) == (
        RuntimeError, "asrx: ctc_weight > 0 needs the CTC head's logits (a model built with ctc=True)")
    assert raised(lambda: m.rescore(s)) == (
        RuntimeError, "asrx: rescoring needs a model with a CTC head (Transformer(..., ctc=True))")
    assert raised(lambda: m.decoder.rescore(None, None)) == (
        RuntimeError, "asrx: rescoring needs the CTC head's logits (a model built with ctc=True)")


def test_ctc_input_takes_plain_tuples():
    from asrx.decode import CtcInput
    assert CtcInput(*("x", 5, 0, None)) == ("x", 5, 0, None, None)
    assert CtcInput(*("x", 5, 0, "len", 60)).V == 60 and CtcInput(*CtcInput("x", 5, 0)).input_lengths is None
