"""ctypes binding of the C-ABI library `libasrx.so`, derived from its header include/asrx.h.

The header is the ABI's only description: it is read once, at import, and its `typedef struct`s, prototypes and
integer `#define`s become the ctypes structures, SIGNATURES / RESTYPES and CONSTS below.  A new entry point needs a
prototype there and a wrapper in kernels.py, nothing here.

Loaded after `import torch` so that the library's libamdhip64.so.7 dependency resolves to the HIP runtime
torch already mapped (both carry SONAME libamdhip64.so.7).  There is NO fallback: if the library is
missing, every op raises.
"""
import ctypes
import keyword
import os
import re

import torch  # noqa: F401  (must be imported first: binds the HIP runtime)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("ASRX_LIB", os.path.join(_HERE, "lib", "libasrx.so"))
HEADER_PATH = os.path.join(os.path.dirname(os.path.dirname(_HERE)), "include", "asrx.h")

c_i32, c_i64, c_u64, c_f32, c_vp = ctypes.c_int32, ctypes.c_int64, ctypes.c_uint64, ctypes.c_float, ctypes.c_void_p

_SCALARS = {"int": c_i32, "int32_t": c_i32, "int64_t": c_i64, "uint64_t": c_u64, "float": c_f32}
# what a data pointer may point to; all of them are passed as c_void_p (an address, a ctypes array, byref() or None)
_POINTEES = {"void", "float", "double", "int32_t", "int64_t", "uint8_t", "uint16_t", "uint32_t"}
# `[const] type[*] name[, name...]`: a parameter, or the fields one struct declaration names
_DECL = re.compile(r"(?:const\s+)?(\w+)\s*(\*?)\s*(\w+(?:\s*,\s*\w+)*)")


def _parse_header(path):
    """(structs, signatures, restypes, consts) of the header: asrx_* struct name -> ctypes.Structure, function name ->
    argtypes / restype, ASRX_* define -> int.  Written for this header's regular style, not for C at large: a type it
    does not know is an error, not a guess."""
    if not os.path.exists(path):
        raise RuntimeError(f"asrx: C-ABI header not found at {path}; the binding is derived from it. "
                           f"There is no fallback table.")
    with open(path) as f:
        text = re.sub(r"/\*.*?\*/", " ", f.read(), flags=re.S)
    structs = {}

    def decl(d):   # -> (names, ctype)
        m = _DECL.fullmatch(d.strip())
        base, ptr, names = m.groups() if m else (None, None, None)
        if ptr == "" and base in _SCALARS:
            ctype = _SCALARS[base]
        elif ptr and base == "char":
            ctype = ctypes.c_char_p
        elif ptr and base in structs:
            ctype = ctypes.POINTER(structs[base])
        elif ptr and base in _POINTEES:
            ctype = c_vp
        else:
            raise RuntimeError(f"asrx: {path}: cannot bind the declaration {d.strip()!r}")
        return [n + "_" if keyword.iskeyword(n) else n for n in re.split(r"\s*,\s*", names)], ctype

    # (field order and names are the header's: kernels.gemm builds its GemmDesc with one positional constructor call)
    for m in re.finditer(r"typedef\s+struct\s+(\w+)\s*\{(.*?)\}\s*\1\s*;", text, re.S):
        fields = []
        for d in filter(str.strip, m.group(2).split(";")):
            names, ctype = decl(d)
            fields += [(n, ctype) for n in names]
        cls = "".join(w.capitalize() for w in m.group(1).split("_")[1:])   # asrx_gemm_desc -> GemmDesc
        structs[m.group(1)] = type(cls, (ctypes.Structure,), {"_fields_": fields, "__module__": __name__})
    signatures, restypes = {}, {}
    for m in re.finditer(r"\b(int|int64_t)\s+(asrx_\w+)\s*\(([^()]*)\)\s*;", text):
        params = m.group(3).strip()
        signatures[m.group(2)] = [] if params == "void" else [decl(p)[1] for p in params.split(",")]
        restypes[m.group(2)] = _SCALARS[m.group(1)]
    unbound = set(re.findall(r"\b(asrx_\w+)\s*\(", text)) - set(signatures)
    if unbound:   # (a result type or a parameter list the pattern above does not take)
        raise RuntimeError(f"asrx: {path}: cannot bind the prototype of {sorted(unbound)}")
    consts = {m.group(1): int(m.group(2))
              for m in re.finditer(r"^#define[ \t]+(ASRX_\w+)[ \t]+\(?(-?\d+)\)?[ \t]*$", text, re.M)}
    return structs, signatures, restypes, consts


# SIGNATURES: name -> argtypes, RESTYPES: name -> restype (int, or int64 for the size helpers), CONSTS: the defines
_STRUCTS, SIGNATURES, RESTYPES, CONSTS = _parse_header(HEADER_PATH)

GemmDesc, AttnDesc, GemmGroupDev, RowsumGroup, AdamDesc = (_STRUCTS["asrx_" + n] for n in (
    "gemm_desc", "attn_desc", "gemm_group_dev", "rowsum_group", "adam_desc"))
GemmGroupDev.__doc__ = "asrx_gemm_group_dev: one 64-byte entry of a grouped launch's device table."

BF16, F32, BITS = CONSTS["ASRX_BF16"], CONSTS["ASRX_F32"], CONSTS["ASRX_BITS"]
CTC_SUM, CTC_MEAN = CONSTS["ASRX_CTC_SUM"], CONSTS["ASRX_CTC_MEAN"]    # asrx_ctc_loss reduction codes
ED_PAIRS, ED_GROUP, ED_CROSS = (CONSTS["ASRX_ED_" + n] for n in ("PAIRS", "GROUP", "CROSS"))   # asrx_edit_distance
NGRAM_MAX_ORDER = CONSTS["ASRX_NGRAM_MAX_ORDER"]
SPECAUG_MAX_MASKS = CONSTS["ASRX_SPECAUG_MAX_MASKS"]
SPECAUG_RUN = CONSTS["ASRX_SPECAUG_RUN"]            # frames one workgroup of asrx_specaug covers
LOGMEL_MAX_MELS = CONSTS["ASRX_LOGMEL_MAX_MELS"]
MAX_ROWSUM_GROUPS = 64      # norm.hip RG_MAX
CTC_MAX_TARGET = 255        # longest target asrx_ctc_loss takes (511 extended states)
CTC_LONG_MAX_TARGET = CONSTS["ASRX_CTC_LONG_MAX_TARGET"]   # ... asrx_ctc_loss_long / asrx_ctc_align_long take
ED_MAX_TOKENS = 255         # longest kept sequence asrx_edit_distance takes
ED_LONG_MAX_TOKENS = CONSTS["ASRX_ED_LONG_MAX_TOKENS"]     # ... asrx_edit_distance_long takes

ERRORS = {CONSTS["ASRX_ERR_ARG"]: "bad argument", CONSTS["ASRX_ERR_LAUNCH"]: "launch failure",
          CONSTS["ASRX_ERR_UNSUPPORTED"]: "unsupported shape/layout"}

_lib = None


def lib():
    """Load (once) and return the ctypes library. Raises if the HIP library was not built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(f"asrx: native library not found at {LIB_PATH}; run __graft_entry__.build() "
                               f"(python -m asrx._build). There is no CPU fallback.")
        L = ctypes.CDLL(LIB_PATH)
        for name, argt in SIGNATURES.items():
            fn = getattr(L, name)
            fn.argtypes = argt
            fn.restype = RESTYPES[name]
        _lib = L
    return _lib


def check(rc, name):
    if rc != 0:
        raise RuntimeError(f"asrx: {name} failed: {ERRORS.get(rc, rc)}")


_FNS = {}


def call(name, *args):
    fn = _FNS.get(name)
    if fn is None:
        fn = _FNS[name] = getattr(lib(), name)
    rc = fn(*args)
    if rc != 0:
        raise RuntimeError(f"asrx: {name} failed: {ERRORS.get(rc, rc)}")
