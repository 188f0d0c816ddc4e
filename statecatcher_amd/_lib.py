"""ctypes binding of libstatecatcher_hip.so (C ABI: include/statecatcher.h).

The header is the one definition of the ABI: every prototype, job struct and `#define SC_*` integer
is read from it at import, so the binding cannot drift from what the library was compiled against.

The product path has no CPU fallback: every op raises if the library is missing, if a tensor is
not on a ROCm device, or if a call returns a non-zero status.
"""
import ctypes
import os
import re

import torch  # noqa: F401  (loads torch's HIP runtime first: our .so binds to the same SONAME)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_NAME = "libstatecatcher_hip.so"
# SC_LIB_PATH: load another build of the same ABI (ablation builds under tools/); default in-tree
LIB_PATH = os.environ.get("SC_LIB_PATH") or os.path.join(_HERE, LIB_NAME)
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "statecatcher.h")

_SCALARS = {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "size_t": ctypes.c_size_t,
            "float": ctypes.c_float, "double": ctypes.c_double}
_RETURNS = dict(_SCALARS, **{"void": None, "const char *": ctypes.c_char_p})
_POINTEES = set(_SCALARS) | {"void", "char", "int32_t", "uint8_t"}   # and the header's own structs
_STRUCT = re.compile(r"typedef\s+struct\s*(\w*)\s*\{([^{}]*)\}\s*(\w+)\s*;")
_PROTO = re.compile(r"(\w[\w\s*]*?)\b(\w+)\s*\(([^(){};]*)\)\s*;")
_DEFINE = re.compile(r"^[ \t]*#[ \t]*define[ \t]+(SC_\w+)\b(.*)$", re.M)
_SPACE = re.compile(r"\s*")
_INTEGER = re.compile(r"\s*(?:(-?\d+)|\(\s*(-?\d+)\s*\))\s*")


def _declare(text, structs, where):
    """`[const] type a, *b` -> [(name, ctype), ...].  Pointers stay untyped: callers pass None, raw
    integer addresses, c_void_p and ctypes arrays."""
    m = re.fullmatch(r"\s*(?:const\s+)?(?:struct\s+)?(\w+)\b(.*)", text, re.S)
    out = []
    for d in m.group(2).split(",") if m else [""]:
        dm = re.fullmatch(r"\s*(\**)\s*(\w*)\s*", d) if m else None
        if not dm or dm.group(2) in ("const", "struct"):
            raise ValueError(f"statecatcher.h: cannot parse {text.strip()!r} in: {where}")
        base, stars, name = m.group(1), dm.group(1), dm.group(2)
        if base not in ((_POINTEES | set(structs)) if stars else _SCALARS):
            raise ValueError(f"statecatcher.h: type of {text.strip()!r} not supported in: {where}")
        out.append((name, ctypes.c_void_p if stars else _SCALARS[base]))
    return out


def parse_header(text):
    """Header text -> (constants {name: int}, structs {name: ctypes.Structure class}, signatures
    {name: (restype, argtypes)}).  Fails closed: a declaration it does not fully understand raises
    ValueError quoting it; nothing is skipped or guessed."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    consts = {}
    for name, value in _DEFINE.findall(text):
        m = _INTEGER.fullmatch(value)
        if not m:
            raise ValueError(f"statecatcher.h: #define {name}{value} is no integer constant")
        consts[name] = int(m.group(1) or m.group(2))
    text = re.sub(r"^[ \t]*#.*$", "", text, flags=re.M)
    text, wrapped = re.subn(r'extern\s+"C"\s*\{', "", text.rstrip(), count=1)
    if wrapped:
        if not text.endswith("}"):
            raise ValueError('statecatcher.h: extern "C" { is never closed')
        text = text[:-1]
    structs, sigs, pos = {}, {}, 0
    while True:
        pos = _SPACE.match(text, pos).end()
        if pos == len(text):
            return consts, structs, sigs
        m = _STRUCT.match(text, pos) or _PROTO.match(text, pos)
        where = " ".join((m.group(0) if m else text[pos:].partition(";")[0]).split())
        if not m:
            raise ValueError(f"statecatcher.h: cannot parse declaration: {where}")
        if m.re is _STRUCT:
            tag, body, name = m.groups()
            fields = [f for part in body.split(";") if part.strip()
                      for f in _declare(part, structs, where)]
            if tag not in ("", name) or not fields or not all(n for n, _ in fields):
                raise ValueError(f"statecatcher.h: cannot parse struct: {where}")
            structs[name] = type(name, (ctypes.Structure,), {
                "_fields_": fields, "__doc__": f"{name} (include/statecatcher.h)."})
        else:
            ret, name, params = m.groups()
            ret = " ".join(ret.replace("*", " * ").split())
            if ret not in _RETURNS:
                raise ValueError(f"statecatcher.h: return type {ret!r} not supported in: {where}")
            params = [] if params.strip() in ("", "void") else params.split(",")
            sigs[name] = (_RETURNS[ret], [_declare(p, structs, where)[0][1] for p in params])
        pos = m.end()


def _read_header():
    try:
        with open(HEADER_PATH) as f:
            return f.read()
    except OSError as e:
        raise RuntimeError(f"statecatcher C ABI header missing: {HEADER_PATH} (the Python binding "
                           f"is derived from it): {e}") from None


CONSTANTS, STRUCTS, _SIGS = parse_header(_read_header())
globals().update(CONSTANTS)   # SC_EINVAL, SC_F32, SC_MAX_FRAME_JOBS, SC_FRAME_PLAIN, ...
EXPORTED = tuple(_SIGS)
ABI_VERSION = CONSTANTS["SC_ABI_VERSION"]   # load() refuses a library built from another header
_DTYPE = {torch.float32: CONSTANTS["SC_F32"], torch.bfloat16: CONSTANTS["SC_BF16"],
          torch.float16: CONSTANTS["SC_F16"]}
AdamTensor = STRUCTS["sc_adam_tensor"]
ImageJob = STRUCTS["sc_image_job"]
LnFoldJob = STRUCTS["sc_ln_fold_job"]
FrameGemmJob = STRUCTS["sc_frame_gemm_job"]
FrameCellJob = STRUCTS["sc_frame_cell_job"]
TFrameJob = STRUCTS["sc_tframe_job"]

_LIB = None


def load():
    """Load (once) and return the ctypes handle.  Raises RuntimeError if it is not built."""
    global _LIB
    if _LIB is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"statecatcher HIP library not built: {LIB_PATH} missing "
                "(run `python -c 'import __graft_entry__ as g; g.build()'` or "
                "`make -C statecatcher_amd/csrc`)")
        lib = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in _SIGS.items():
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
        if lib.sc_abi_version() != ABI_VERSION:
            raise RuntimeError("statecatcher ABI version mismatch")
        _LIB = lib
    return _LIB


def check(rc, what):
    if rc != 0:
        msg = load().sc_last_error().decode(errors="replace")
        if rc < 0:
            raise ValueError(f"{what}: {msg}")
        raise RuntimeError(f"{what}: HIP error {rc}: {msg}")


def dtype_code(t):
    try:
        return _DTYPE[t.dtype]
    except KeyError:
        raise TypeError(f"unsupported dtype {t.dtype}; expected float32, bfloat16 or float16") from None


def require_device(*tensors):
    for t in tensors:
        if t is not None and t.device.type != "cuda":
            raise RuntimeError(
                "statecatcher ops run only on a ROCm GPU (HIP); got a tensor on "
                f"{t.device}. There is no CPU fallback.")


def stream_of(t):
    return ctypes.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)


def ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None
