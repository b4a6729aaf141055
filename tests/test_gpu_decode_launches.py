"""The launch sequence of every decoding mode, pinned: each public decoding entry point must issue exactly the native
calls, with exactly the scalar arguments, that tests/golden/decode_calls.json records.  Decoding is bound by the host
(DESIGN.md §8), so "the same launches in the same order" is the property a restructuring of the drivers has to keep;
the results themselves are held to the oracles by test_gpu_beam_model.py and its neighbours.

What is recorded per call of asrx.kernels.call: the entry point's name and its non-address arguments.  Which those are
is read from asrx._lib.SIGNATURES: scalar positions are kept; `void*` positions (device addresses, the stream) are
dropped, as they differ from run to run; a descriptor passed by reference (asrx_gemm, asrx_attention_fwd) contributes
its non-pointer fields, its pointer fields being dropped for the same reason.  Nothing else is left out.  The fixture
keeps every name in full and one digest of the scalars per call.

The fixture is written by running this module as a script on the tree whose launches are to be kept:

    python tests/test_gpu_decode_launches.py tests/golden/decode_calls.json

Model: c1 (d 128) as test_gpu_beam_model.py builds it, with a CTC head for the CTC cases; the LM of
test_gpu_ngram_model.py; B = 2, Te = 24, 3 new tokens."""
import ctypes
import functools
import hashlib
import json
import os
import struct
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
dev = "cuda"
HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "decode_calls.json")
EOS, MAX_LEN, B, TE = 22, 3, 2, 24


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


# ------------------------------------------------------------------------------------------- recording

def _f32(x):
    return struct.unpack("f", struct.pack("f", float(x)))[0]


def _value(ctype, v):
    v = getattr(v, "value", v)
    return _f32(v) if ctype is ctypes.c_float else int(v)


def scalars(name, args):
    """The non-address arguments of one call, in order; a descriptor becomes the dict of its non-pointer fields."""
    from asrx._lib import SIGNATURES
    out = []
    for ctype, a in zip(SIGNATURES[name], args):
        if issubclass(ctype, ctypes._SimpleCData) and ctype not in (ctypes.c_void_p, ctypes.c_char_p):
            out.append(_value(ctype, a))
        elif hasattr(a, "_obj"):                                    # byref(descriptor)
            d = a._obj
            out.append({f: _value(t, getattr(d, f)) for f, t in d._fields_ if t is not ctypes.c_void_p})
    return out


def digest(values):
    return hashlib.sha1(json.dumps(values).encode()).hexdigest()[:12]


def record(fn):
    """[(name, scalars)] of the native calls fn() issues.  fn runs once unrecorded first, so that what a first call
    on a fresh model sets up (the flat parameter store) is no part of any case, whatever ran before it."""
    from asrx import kernels as K
    with torch.no_grad():
        fn()
        calls, real = [], K.call
        K.call = lambda name, *a: (calls.append((name, scalars(name, a))), real(name, *a))[1]
        try:
            fn()
        finally:
            K.call = real
    torch.cuda.synchronize()
    return calls


# ------------------------------------------------------------------------------------------- models and inputs

@functools.lru_cache(maxsize=None)
def params(zero_classifier=False):
    from oracle.ref_model import CONFIGS, det_params
    cfg = CONFIGS["c1"]["cfg"]
    P = det_params(cfg, 3)
    P["decoder._classifier.weight"] = P["decoder._classifier.weight"] * (0 if zero_classifier else 4)
    return cfg, P


@functools.lru_cache(maxsize=None)
def model(ctc=False, mask_padding=False, zero_classifier=False):
    import asrx
    cfg, P = params(zero_classifier)
    torch.manual_seed(7)                # (the CTC head is not among the oracle's parameters: its own init)
    m = asrx.Transformer(cfg.vocab_size, cfg.input_dim, cfg.d_model, cfg.dec_len, cfg.enc_len, cfg.n_enc, cfg.n_dec,
                         cfg.n_heads, cfg.ff_dim, dropout=cfg.dropout, precision="fp32", ctc=ctc,
                         mask_padding=mask_padding)
    sd = m.state_dict()
    sd.update(P)
    m.load_state_dict(sd)
    m = m.to(dev).eval()
    m.decoder._eos_token_id = 0 if zero_classifier else EOS
    return m


@functools.lru_cache(maxsize=None)
def language_model():
    import asrx
    cfg, _ = params()
    g = torch.Generator().manual_seed(0)
    corpus = []
    for _ in range(40):
        n = int(torch.randint(2, 8, (1,), generator=g))
        corpus.append(torch.randint(5, 60, (n,), generator=g).tolist())
    return asrx.NgramLM.estimate(corpus, 3, cfg.vocab_size, bos_id=1, eos_id=EOS, exclude=(cfg.pad_id,),
                                 discount=0.75).to(dev)


@functools.lru_cache(maxsize=None)
def inputs():
    cfg, _ = params()
    g = torch.Generator().manual_seed(7)
    enc = torch.randn(B, TE, cfg.d_model, generator=g).to(dev)
    ctc_logits = torch.randn(B * TE, cfg.vocab_size, generator=g).to(dev)
    spectrum = torch.randn(B, 1, cfg.input_dim, 100, generator=g).to(dev)       # 100 frames -> Te = 24
    return dict(enc=enc, bos=torch.ones(B, 1, dtype=torch.int64, device=dev),
                prompt3=torch.tensor([[1, 7, 9], [1, 11, 5]], dtype=torch.int64, device=dev),
                ctc=(ctc_logits, TE, cfg.pad_id, None), spectrum=spectrum,
                lengths=torch.tensor([TE, 17], dtype=torch.int32, device=dev))


def _evaluate(prompt):
    def run():
        dec = model().decoder
        keep, dec._seq_len = dec._seq_len, MAX_LEN
        try:
            return dec.evaluate(inputs()[prompt], inputs()["enc"])
        finally:
            dec._seq_len = keep
    return run


def _resolve(kw):
    """The keyword arguments of a case, its placeholders replaced by the shared inputs."""
    kw = dict(kw)
    if "ctc_weight" in kw:
        kw["ctc"] = inputs()["ctc"]
    if "lm" in kw:
        kw["lm"] = language_model()
    if "enc_lengths" in kw:
        kw["enc_lengths"] = inputs()["lengths"]
    return kw


def _beam(beam=3, zero=False, max_len=MAX_LEN, **kw):
    def run():
        m = model(ctc="ctc_weight" in kw, zero_classifier=zero)
        return m.decoder.beam_search(inputs()["bos"], inputs()["enc"], beam=beam, max_len=max_len, nbest=beam,
                                     **_resolve(kw))
    return run


def _rescore(**kw):
    def run():
        i = inputs()
        return model(ctc=True).decoder.rescore(i["enc"], i["ctc"], beam=3, nbest=3, max_len=MAX_LEN, **_resolve(kw))
    return run


def _front_door():
    i = inputs()
    return model(ctc=True, mask_padding=True).beam_search(i["spectrum"], beam=3, max_len=MAX_LEN, ctc_weight=0.3,
                                                          input_lengths=i["lengths"], poll=0)


CASES = {
    "evaluate prompt 1": _evaluate("bos"),
    "evaluate prompt 3": _evaluate("prompt3"),
    "beam 1": _beam(1, poll=0),
    "beam 3": _beam(poll=0),
    # (all three hypotheses of the zero-classifier model are finished after three steps, and the poll only stops a
    # search that has steps left: this one case asks for a fourth)
    "beam 3 poll 1 early stop": _beam(zero=True, poll=1, max_len=MAX_LEN + 1),
    "beam 3 no final norm": _beam(poll=0, final_norm=False),
    "beam 3 ctc": _beam(poll=0, ctc_weight=0.3),
    "beam 3 lm": _beam(poll=0, lm=True, lm_weight=0.5),
    "beam 3 ctc lm bonus": _beam(poll=0, ctc_weight=0.3, lm=True, lm_weight=0.5, token_bonus=0.2),
    "beam 3 enc_lengths": _beam(poll=0, enc_lengths=True),
    "rescore": _rescore(),
    "rescore mbr": _rescore(mbr_scale=1.0),
    "rescore lm": _rescore(lm=True, lm_weight=0.5, token_bonus=0.2),
    "rescore enc_lengths": _rescore(enc_lengths=True),
    "transformer beam 3 ctc mask_padding": _front_door,
}


# ------------------------------------------------------------------------------------------- the test

@functools.lru_cache(maxsize=None)
def fixture():
    with open(FIXTURE) as f:
        return json.load(f)


@pytest.mark.parametrize("case", list(CASES))
def test_decode_issues_the_recorded_launches(case):
    want = fixture()[case]
    got = record(CASES[case])
    assert len(want) > 0
    for n, ((name, values), line) in enumerate(zip(got, want)):
        assert f"{name} {digest(values)}" == line, f"{case}: call {n} is {name}{values}, recorded as {line}"
    assert [name for name, _ in got] == [line.split()[0] for line in want]


def test_the_early_stop_case_stops_early():
    """The poll = 1 case asks for four steps and must leave after three, or it records no early stop."""
    steps = sum(line.startswith("asrx_beam_step") for line in fixture()["beam 3 poll 1 early stop"])
    assert steps == MAX_LEN


if __name__ == "__main__":
    repo = os.path.dirname(HERE)
    sys.path[:0] = [repo, os.path.join(repo, "asr-transformer_amd")]
    out = {case: [f"{name} {digest(values)}" for name, values in record(fn)] for case, fn in CASES.items()}
    path = sys.argv[1] if len(sys.argv) > 1 else FIXTURE
    with open(path, "w") as f:
        json.dump(out, f, indent=0)
        f.write("\n")
    print({case: len(lines) for case, lines in out.items()})
