"""CPU-side checks of the feature-normalisation entry points (include/ltrx.h, allrank_amd/csrc/ltrx_featnorm.hip): declared, bound from
the header, exported by the built library, refusing bad arguments before any HIP call, workspace sizes monotone in the row count -- and
the Python launchers of allrank_amd/normalize.py held to the header's parameter names with a recording stand-in for the library.
No kernel is launched."""
import ast
import ctypes
import os
import re

import pytest
import torch

FAKE = ctypes.c_void_p(4096)                            # never dereferenced: the argument checks come first
HOST = ctypes.c_double(1e-2)
AT = ctypes.c_void_p(ctypes.addressof(HOST))
NAMES = ("ltrx_feature_min_workspace_bytes", "ltrx_feature_min", "ltrx_feature_moments_workspace_bytes", "ltrx_feature_moments",
         "ltrx_feature_normalize")


@pytest.fixture(scope="module")
def lib():
    from allrank_amd import _lib, build
    build.build(verbose=False)
    return _lib.lib()


def _params(name):
    from allrank_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(_lib.HEADER_PATH).read(), flags=re.S)
    params = re.search(r"\b%s\s*\(([^()]*)\)" % name, src).group(1)
    return [re.search(r"(\w+)\s*$", q).group(1) for q in params.split(",")]


def test_the_prototypes_are_declared_bound_and_exported(lib):
    from allrank_amd import _lib
    h = ctypes.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert name in _lib.SIGNATURES and hasattr(h, name) and hasattr(lib, name), name
        res, args = _lib.SIGNATURES[name]
        assert len(args) == len(_params(name))
        query = name.endswith("_bytes")
        assert res is (ctypes.c_size_t if query else ctypes.c_int)
        assert (_lib.PROTOTYPES[name][1][-1] == "ltrx_stream_t") == (not query)
    assert _params("ltrx_feature_min") == ["x", "n", "F", "ld", "negate", "min_out", "ws", "stream"]
    assert _params("ltrx_feature_moments") == ["x", "n", "F", "ld", "negate", "take_log", "eps_log_host", "mean_out", "std_out", "ws", "stream"]
    assert _params("ltrx_feature_normalize") == ["x", "n", "F", "ld", "negate", "take_log", "eps_log_host", "mean", "std", "eps_host", "stream"]
    assert lib.ltrx_version() == 130


def _min(lib, x=FAKE, n=5, F=3, ld=3, negate=FAKE, out=FAKE, ws=FAKE):
    return lib.ltrx_feature_min(x, n, F, ld, negate, out, ws, None)


def _moments(lib, x=FAKE, n=5, F=3, ld=3, negate=FAKE, take_log=FAKE, eps_log=AT, mean=FAKE, std=FAKE, ws=FAKE):
    return lib.ltrx_feature_moments(x, n, F, ld, negate, take_log, eps_log, mean, std, ws, None)


def _normalize(lib, x=FAKE, n=5, F=3, ld=3, negate=FAKE, take_log=FAKE, eps_log=AT, mean=FAKE, std=FAKE, eps=AT):
    return lib.ltrx_feature_normalize(x, n, F, ld, negate, take_log, eps_log, mean, std, eps, None)


@pytest.mark.parametrize("call", [_min, _moments, _normalize])
def test_bad_shapes_are_invalid(lib, call):
    for bad in (dict(x=None), dict(negate=None), dict(n=0), dict(n=-4), dict(F=0), dict(F=-1), dict(F=4, ld=3), dict(ld=0)):
        assert call(lib, **bad) == -1, bad


def test_null_operands_are_invalid(lib):
    for bad in ("out", "ws"):
        assert _min(lib, **{bad: None}) == -1, bad
    for bad in ("take_log", "eps_log", "mean", "std", "ws"):
        assert _moments(lib, **{bad: None}) == -1, bad
    for bad in ("take_log", "eps_log", "mean", "std", "eps"):
        assert _normalize(lib, **{bad: None}) == -1, bad


@pytest.mark.parametrize("query", ["ltrx_feature_min_workspace_bytes", "ltrx_feature_moments_workspace_bytes"])
def test_workspace_sizes_are_monotone_in_the_row_count(lib, query):
    fn = getattr(lib, query)
    for F in (1, 3, 46, 136, 137, 700):
        sizes = [fn(n, F) for n in (1, 2, 63, 64, 65, 257, 4097, 100000, 2270000, 2 ** 31 - 1)]
        assert sizes == sorted(sizes) and sizes[0] >= F * 8, (F, sizes)       # at least one row of F doubles
        assert sizes[-1] == sizes[-2], (F, sizes)                             # bounded: the workgroup count is
        assert fn(4097, F + 1) > fn(4097, F)
    assert fn(0, 5) == 0 and fn(5, 0) == 0 and fn(-1, 5) == 0


# ---- the Python launchers ---------------------------------------------------------------------------------------------
class Recorder(object):
    """stands in for the bound library: records (name, arguments) -- a pointer as its address, or for the parameters named in
    ``reads`` as the double found there WHILE the call runs -- and returns 0 or ``returns[name]``"""

    def __init__(self, returns=None, reads=()):
        self.calls, self.returns, self.reads = [], returns or {}, reads

    def __getattr__(self, name):
        def call(*args):
            plain = []
            for pname, a in zip(_params(name), args):
                if isinstance(a, ctypes.c_void_p):
                    a = ctypes.c_double.from_address(a.value).value if pname in self.reads else a.value
                plain.append(a)
            self.calls.append((name, plain))
            return self.returns.get(name, 0)
        return call


def _expect(rec, name, **by_name):
    assert [c[0] for c in rec.calls] == [name], rec.calls
    args = rec.calls[0][1]
    assert list(by_name) == _params(name) and len(args) == len(by_name), (name, len(args))
    for (pname, want), got in zip(by_name.items(), args):
        assert got == want and type(got) is type(want), (name, pname, got, want)


def test_launchers_pass_every_parameter_by_its_header_name():
    from allrank_amd import normalize as N
    st = ctypes.c_void_p(0x5EED)
    x = torch.zeros((9, 16), dtype=torch.float32)[:, :12]                       # 7 of 9 rows, 12 columns, row stride 16
    neg, lg = torch.zeros(12, dtype=torch.uint8), torch.zeros(12, dtype=torch.uint8)
    f64 = lambda: torch.zeros(12, dtype=torch.float64)  # noqa: E731
    mn, mean, std, ws = torch.zeros(12), f64(), f64(), torch.zeros(64, dtype=torch.uint8)
    rec = Recorder()
    N.feature_min(rec, st, x, 7, neg, mn, ws)
    _expect(rec, "ltrx_feature_min", x=x.data_ptr(), n=7, F=12, ld=16, negate=neg.data_ptr(), min_out=mn.data_ptr(), ws=ws.data_ptr(),
            stream=st.value)
    rec = Recorder(reads=("eps_log_host",))
    N.feature_moments(rec, st, x, 7, neg, lg, 0.125, mean, std, ws)
    _expect(rec, "ltrx_feature_moments", x=x.data_ptr(), n=7, F=12, ld=16, negate=neg.data_ptr(), take_log=lg.data_ptr(), eps_log_host=0.125,
            mean_out=mean.data_ptr(), std_out=std.data_ptr(), ws=ws.data_ptr(), stream=st.value)
    rec = Recorder(reads=("eps_log_host", "eps_host"))
    N.feature_normalize(rec, st, x, 7, neg, lg, 0.125, mean, std, 0.5)
    _expect(rec, "ltrx_feature_normalize", x=x.data_ptr(), n=7, F=12, ld=16, negate=neg.data_ptr(), take_log=lg.data_ptr(),
            eps_log_host=0.125, mean=mean.data_ptr(), std=std.data_ptr(), eps_host=0.5, stream=st.value)
    for query, helper in (("ltrx_feature_min_workspace_bytes", N.feature_min_workspace),
                          ("ltrx_feature_moments_workspace_bytes", N.feature_moments_workspace)):
        rec = Recorder(returns={query: 1000})
        got = helper(rec, 7, 12, x)
        _expect(rec, query, n=7, F=12)
        assert got.dtype == torch.uint8 and got.numel() == 1000


def test_each_feature_call_is_written_once_in_the_package():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    seen = {}
    for dirpath, _, files in os.walk(os.path.join(root, "allrank_amd")):
        for f in files:
            if f.endswith(".py"):
                path = os.path.join(dirpath, f)
                for node in ast.walk(ast.parse(open(path).read(), path)):
                    if isinstance(node, ast.Call) and isinstance(node.func, ast.Attribute) and node.func.attr in NAMES:
                        seen.setdefault(node.func.attr, []).append(os.path.relpath(path, root))
    assert seen == {name: [os.path.join("allrank_amd", "normalize.py")] for name in NAMES}, seen
