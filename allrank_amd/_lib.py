"""ctypes binding of libltrx.so (include/ltrx.h).  No fallback: if the library is missing, importing the
kernels fails loudly (the product path never routes through a CPU implementation)."""
import ctypes
import os
import re

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("LTRX_LIB_PATH") or os.path.join(_HERE, "libltrx.so")     # (override: A/B runs of two builds)

HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "ltrx.h")

# C type -> ctypes type.  "*" stands for any pointer, device or host: like ltrx_stream_t it is passed as a raw address.
_CTYPES = {"*": ctypes.c_void_p, "ltrx_stream_t": ctypes.c_void_p, "int": ctypes.c_int, "float": ctypes.c_float,
           "size_t": ctypes.c_size_t, "int32_t": ctypes.c_int32, "uint32_t": ctypes.c_uint32, "uint64_t": ctypes.c_uint64, "int64_t": ctypes.c_int64}


def _ctype_name(decl, where):
    """the key into ``_CTYPES`` of one C declarator (``const float* x`` -> ``*``, ``int n`` -> ``int``)"""
    words = ["*"] if "*" in decl else [w for w in decl.split() if w != "const"]
    if not 1 <= len(words) <= 2 or words[0] not in _CTYPES:
        raise TypeError("include/ltrx.h: no ctypes mapping for %r in %r" % (decl.strip(), where))
    return words[0]


def parse_header(text):
    """{name: (return type, [parameter types])}, as keys of ``_CTYPES``, of every ``ltrx_*`` prototype in the text of
    include/ltrx.h.  An ``ltrx_name(`` outside a readable prototype, or a type outside ``_CTYPES``, raises: the table never guesses."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    text = re.sub(r"^[ \t]*#(?:[^\n]*\\\n)*[^\n]*", " ", text, flags=re.M)
    protos = {m.start(2): m for m in re.finditer(r"([\w\s\*]+?)\b(ltrx_\w+)\s*\(([^()]*)\)\s*;", text)}
    out = {}
    for use in re.finditer(r"\bltrx_\w+\s*\(", text):
        if use.start() not in protos:
            raise TypeError("include/ltrx.h: cannot read the declaration at %r" % " ".join(text[use.start():use.start() + 160].split()))
        ret, name, params = protos[use.start()].groups()
        params = [] if params.strip() in ("", "void") else params.split(",")
        out[name] = (_ctype_name(ret, name), [_ctype_name(q, name) for q in params])
    return out


with open(HEADER_PATH) as _f:
    PROTOTYPES = parse_header(_f.read())
SIGNATURES = {name: (_CTYPES[ret], [_CTYPES[q] for q in params]) for name, (ret, params) in PROTOTYPES.items()}

_lib = None
MAX_SLATE_LEN = 2048            # LTRX_MAX_SLATE_LEN (include/ltrx.h; checked against the header by tests/test_abi.py)
MAX_LONG_SLATE_LEN = 16384      # LTRX_MAX_LONG_SLATE_LEN: listNet / listMLE / approxNDCG / lambdaLoss (work arrays in the workspace beyond LDS)
MAX_METRIC_SLATE_LEN = 8192     # LTRX_MAX_METRIC_SLATE_LEN


class _Stream(ctypes.c_void_p):
    """a hipStream_t that remembers the device it belongs to (``launch_stream`` / ``stream_of``)"""
    dev = None


class _Bound(object):
    """namespace of the bound entry points (attribute access like a ctypes.CDLL)"""


def _on_stream_device(fn):
    """Entry points that take a stream launch on it; HIP requires the stream's device to be the CURRENT device.  The stream
    argument produced by ``stream_of`` / ``launch_stream`` carries its device; when that is not the current device (explicit
    cuda:1 tensors while cuda:0 is current -- plain user code after the reference's DataParallel gather, or replica threads)
    the launch is wrapped in a device guard.  Every launch made with that stream object is guarded, not only the first
    (ADVICE r2).  A raw / NULL stream is left alone."""
    def call(*args):
        dev = getattr(args[-1], "dev", None) if args else None
        if dev is None or dev == torch.cuda.current_device():
            return fn(*args)
        with torch.cuda.device(dev):
            return fn(*args)
    call.__name__ = fn.__name__
    return call


def lib():
    """The loaded library (loads on first use).  Raises if libltrx.so has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                "allrank_amd: %s is missing -- build it with `python -m allrank_amd.build` "
                "(there is no CPU fallback for the HIP kernels)" % LIB_PATH)
        h = ctypes.CDLL(LIB_PATH)
        b = _Bound()
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(h, name)     # AttributeError if the symbol is not exported
            fn.restype = res
            fn.argtypes = args
            setattr(b, name, _on_stream_device(fn) if PROTOTYPES[name][1][-1:] == ["ltrx_stream_t"] else fn)
        _lib = b
    return _lib


def check(rc, what):
    if rc != 0:
        kinds = {-1: "invalid argument",
                 -2: "unsupported shape (slate length above LTRX_MAX_SLATE_LEN = %d for a loss -- LTRX_MAX_LONG_SLATE_LEN = %d for listNet / "
                     "listMLE / approxNDCGLoss / lambdaLoss -- or LTRX_MAX_METRIC_SLATE_LEN = %d for a metric, or an alignment the kernel "
                     "needs -- see include/ltrx.h; there is no fallback path)" % (MAX_SLATE_LEN, MAX_LONG_SLATE_LEN, MAX_METRIC_SLATE_LEN)}
        msg = kinds.get(rc, "HIP error %d" % (-rc - 1000) if rc <= -1000 else "error")
        raise RuntimeError("libltrx %s failed: %s (code %d)" % (what, msg, rc))


def ptr(t):
    """raw device address of a tensor (None -> NULL)."""
    if t is None:
        return None
    return ctypes.c_void_p(t.data_ptr())


def launch_stream(device):
    """torch's current stream on ``device`` as a hipStream_t that carries its device for the launch guard of ``lib()``."""
    device = torch.device(device)
    st = _Stream(torch.cuda.current_stream(device).cuda_stream)
    st.dev = device.index if device.index is not None else torch.cuda.current_device()
    return st


def stream_of(t):
    return launch_stream(t.device)


def require_device(*tensors):
    dev = None
    for t in tensors:
        if t is None:
            continue
        if not t.is_cuda:
            raise RuntimeError("allrank_amd kernels run on the MI355X only: got a %s tensor (no CPU fallback; "
                               "use the reference implementation on CPU)" % t.device)
        if dev is None:
            dev = t.device
        elif t.device != dev:
            raise RuntimeError("allrank_amd kernels need all tensors of a call on one device: got %s and %s" % (dev, t.device))


def workspace(nbytes, like):
    return torch.empty(max(int(nbytes), 64), dtype=torch.uint8, device=like.device)


def f32c(t):
    """contiguous float32 view/copy"""
    if t.dtype != torch.float32:
        t = t.float()
    return t.contiguous()
