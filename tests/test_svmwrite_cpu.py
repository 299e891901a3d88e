"""CPU-side checks of the libsvm writer (allrank_amd/saving.py, allrank_amd/csrc/ltrx_fmt.h, ltrx_svmwrite.hip; include/ltrx.h,
"libsvm text written on the device"): the exact %.16g formatter through its host-only hook, the host path against the reference's
own files (tests/golden/svmwrite_golden.npz), the refusals, install(saving=True), the two launchers held to the header's parameter
names with a recording stand-in, and the fixture's drift guard.  No kernel is launched."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from oracle.ref_loader import reference_available
from tests.golden import make_golden_svmwrite as G

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "svmwrite_golden.npz")
SLOT = 24


@pytest.fixture(scope="module")
def lib():
    from allrank_amd import _lib, build
    build.build(verbose=False)
    return _lib.lib()


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture
def host_only(monkeypatch):
    """the writer as a machine without a GPU runs it"""
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)


# ---- the formatting core -----------------------------------------------------------------------------------------------
def _texts(lib, v):
    v = np.ascontiguousarray(v, dtype=np.float32)
    text = np.full(v.size * SLOT, 0x7F, dtype=np.uint8)
    n = np.full(v.size, -1, dtype=np.int32)
    assert lib.ltrx_debug_format_g16(v.ctypes.data, v.size, text.ctypes.data, n.ctypes.data) == 0
    assert n.min() >= 1 and n.max() <= 22
    raw = text.tobytes()
    return [raw[i * SLOT:i * SLOT + k].decode("ascii") for i, k in enumerate(n.tolist())], text.reshape(-1, SLOT), n


def _same_as_python(lib, v):
    got, slots, n = _texts(lib, v)
    want = ["%.16g" % float(x) for x in np.asarray(v, dtype=np.float32)]
    wrong = [(float(x), g, w) for x, g, w in zip(v, got, want) if g != w]
    assert not wrong, (len(wrong), wrong[:5])
    assert (slots[np.arange(SLOT)[None, :] >= n[:, None]] == 0x7F).all()          # nothing behind the text is touched


def test_edge_values_print_as_python_prints_them(lib):
    _same_as_python(lib, G.EDGE)
    _same_as_python(lib, -G.EDGE)
    got, _, _ = _texts(lib, np.asarray([2.0 ** -24, 2.0 ** -23, 0.0, -0.0, np.nan, np.inf, -np.inf, 1e15, 1e16, 0.1], dtype=np.float32))
    assert got == ["5.960464477539062e-08", "1.192092895507812e-07", "0", "-0", "nan", "inf", "-inf", "999999986991104",
                   "1.000000027256422e+16", "0.1000000014901161"]


def test_every_power_of_two(lib):
    k = np.arange(-149, 128)
    p = np.ldexp(1.0, k).astype(np.float32)
    assert (p > 0).all() and np.isfinite(p).all()
    _same_as_python(lib, np.concatenate([p, -p]))


def test_small_mantissas_where_the_exact_ties_live(lib):
    m, e = np.meshgrid(np.arange(1, 65), np.arange(-60, 1), indexing="ij")
    _same_as_python(lib, np.ldexp(m.astype(np.float64), e).astype(np.float32).ravel())


def test_a_million_random_bit_patterns(lib):
    bits = np.random.default_rng(16).integers(0, 2 ** 32, 2 ** 20, dtype=np.uint64).astype(np.uint32)
    v = bits.view(np.float32)
    assert (~np.isfinite(v)).sum() > 1000                    # NaNs and infinities are in the draw
    _same_as_python(lib, v)


def test_bad_arguments_of_the_entry_points_are_invalid(lib):
    fake = ctypes.c_void_p(4096)                             # never dereferenced: the argument checks come first
    assert lib.ltrx_debug_format_g16(None, 1, fake, fake) == -1 and lib.ltrx_debug_format_g16(fake, -1, fake, fake) == -1
    assert lib.ltrx_debug_format_g16(fake, 0, fake, fake) == 0
    ok = dict(X=fake, ldx=8, y=fake, qid=fake, n_rows=3, F=5, pad_value=-1.0, index_base=0)
    for bad in (dict(X=None), dict(y=None), dict(qid=None), dict(n_rows=0), dict(F=0), dict(ldx=4), dict(index_base=-1),
                dict(F=2 ** 31 - 1, ldx=2 ** 31, index_base=1)):
        a = dict(ok, **bad)
        head = (a["X"], a["ldx"], a["y"], a["qid"], a["n_rows"], a["F"], a["pad_value"], a["index_base"])
        assert lib.ltrx_libsvm_line_bytes(*head, fake, fake, None) == -1, bad
        assert lib.ltrx_libsvm_format(*head, fake, 100, fake, None) == -1, bad
    head = tuple(ok.values())
    assert lib.ltrx_libsvm_line_bytes(*head, None, fake, None) == -1 and lib.ltrx_libsvm_line_bytes(*head, fake, None, None) == -1
    assert lib.ltrx_libsvm_format(*head, None, 100, fake, None) == -1 and lib.ltrx_libsvm_format(*head, fake, 100, None, None) == -1
    assert lib.ltrx_libsvm_format(*head, fake, 0, fake, None) == -1


# ---- the host path -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F", G.FS)
def test_host_path_writes_the_references_bytes(golden, host_only, tmp_path, F):
    from allrank_amd import saving as S
    x, y, want = golden["F%d.x" % F], golden["F%d.y" % F], golden["F%d.text" % F].tobytes()
    X, Y = G.slate_list(x, y, golden["lens"], golden["as_torch"])
    path = tmp_path / "list.svm"
    S.write_to_libsvm_without_masked(str(path), X, Y)
    assert path.read_bytes() == want
    assert S.last_run == {"engine": "host", "reason": "no GPU", "rows": int((y != -1).sum()), "bytes": len(want)}
    S.write_to_libsvm_without_masked(str(path), iter(X), (v for v in Y))             # any iterable, as the reference takes
    assert path.read_bytes() == want
    S.write_slates(str(tmp_path / "cube.svm"), torch.from_numpy(x), y)               # the same slates as [N, L, F]
    assert (tmp_path / "cube.svm").read_bytes() == want
    assert sorted(p.name for p in tmp_path.iterdir()) == ["cube.svm", "list.svm"]    # no temporary file stays behind
    if F == 20:
        assert b"\n2.5 qid:0 \n" in want and b"qid:1 " not in want and b"qid:10 " in want


def test_first_qid_and_labels_that_fp32_does_not_hold(host_only, tmp_path):
    from allrank_amd import saving as S
    x = np.asarray([[[1.0, 0.0, -0.0], [0.0, 0.25, 3.0]], [[0.0, 0.0, 0.0], [7.0, 7.0, 7.0]]], dtype=np.float32)
    y = np.asarray([[0.1, -1.0], [3.0, 1e-3]], dtype=np.float64)
    S.write_slates(str(tmp_path / "a.svm"), x, y, first_qid=41)
    assert (tmp_path / "a.svm").read_bytes() == b"0.1 qid:41 0:1\n3 qid:42 \n0.001 qid:42 0:7 1:7 2:7\n"
    assert not S._exact_in_fp32(y) and S._exact_in_fp32(y.astype(np.float32)) and S._exact_in_fp32(np.asarray([3, 1 << 24]))
    assert not S._exact_in_fp32(np.asarray([(1 << 24) + 1]))
    S.write_slates(str(tmp_path / "i.svm"), x.astype(np.int64), np.asarray([[2, -1], [-1, 0]]))          # integers print as integers
    assert (tmp_path / "i.svm").read_bytes() == b"2 qid:0 0:1\n0 qid:1 0:7 1:7 2:7\n"
    S.write_slates(str(tmp_path / "f0.svm"), np.zeros((1, 2, 0), dtype=np.float32), np.asarray([[1.5, -1.0]], dtype=np.float32))
    assert (tmp_path / "f0.svm").read_bytes() == b"1.5 qid:0 \n" and S.last_run["reason"] == "no GPU"


def test_refusals_leave_no_file(host_only, tmp_path):
    from allrank_amd import saving as S
    x = np.ones((2, 3, 4), dtype=np.float32)
    y = np.asarray([[1, 0, -1], [2, -1, -1]], dtype=np.float32)
    path = tmp_path / "out.svm"
    for where, what in (((0, 1, 2), np.nan), ((1, 0, 0), np.inf), ((0, 0, 3), -np.inf)):
        bad = x.copy()
        bad[where] = what
        with pytest.raises(ValueError, match="NaN or an infinity"):
            S.write_slates(str(path), bad, y)
        assert list(tmp_path.iterdir()) == []
    ybad = y.copy()
    ybad[1, 0] = np.nan
    with pytest.raises(ValueError, match="NaN or an infinity"):
        S.write_slates(str(path), x, ybad)
    with pytest.raises(ValueError, match="no row to write"):
        S.write_slates(str(path), x, np.full_like(y, -1.0))
    with pytest.raises(ValueError, match="no row to write"):
        S.write_to_libsvm_without_masked(str(path), [x[0], x[1]], [np.full(3, -1.0, dtype=np.float32)] * 2)
    with pytest.raises(ValueError, match="no row to write"):
        S.write_to_libsvm_without_masked(str(path), [], [])
    assert list(tmp_path.iterdir()) == []
    bad = x.copy()
    bad[0, 2], bad[1, 1, 0] = np.nan, np.inf                 # padded rows: not an error
    S.write_slates(str(path), bad, y)
    assert path.read_bytes() == b"1 qid:0 0:1 1:1 2:1 3:1\n0 qid:0 0:1 1:1 2:1 3:1\n2 qid:1 0:1 1:1 2:1 3:1\n"


# ---- install(saving=True) ------------------------------------------------------------------------------------------------
@pytest.mark.skipif(not reference_available(), reason="reference tree only exists in the build container")
def test_install_saving_rebinds_both_names_and_uninstall_restores():
    import importlib
    import inspect
    from oracle.ref_loader import load_reference
    load_reference()
    import allrank.data.dataset_saving as RS
    import allrank_amd
    from allrank_amd import saving as S
    rc = importlib.import_module("allrank.rank_and_click")
    ref = RS.write_to_libsvm_without_masked
    assert rc.write_to_libsvm_without_masked is ref
    assert list(inspect.signature(S.write_to_libsvm_without_masked).parameters) == list(inspect.signature(ref).parameters)
    try:
        allrank_amd.install()                                # a bare install() leaves the writer alone
        assert RS.write_to_libsvm_without_masked is ref and rc.write_to_libsvm_without_masked is ref
        allrank_amd.uninstall()
        done = allrank_amd.install(saving=True)
        assert RS.write_to_libsvm_without_masked is S.write_to_libsvm_without_masked
        assert rc.write_to_libsvm_without_masked is S.write_to_libsvm_without_masked
        assert inspect.signature(S.write_to_libsvm_without_masked) == inspect.signature(ref)
        assert {"allrank.data.dataset_saving.write_to_libsvm_without_masked",
                "allrank.rank_and_click.write_to_libsvm_without_masked"} <= set(done)
        assert not [n for n in done if n.endswith((".rank_slates", ".click_on_slates"))]          # independent of inference / clicks
    finally:
        allrank_amd.uninstall()
    assert RS.write_to_libsvm_without_masked is ref and rc.write_to_libsvm_without_masked is ref


# ---- the Python launchers ---------------------------------------------------------------------------------------------
def _params(name):
    from allrank_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(_lib.HEADER_PATH).read(), flags=re.S)
    params = re.search(r"\b%s\s*\(([^()]*)\)" % name, src).group(1)
    return [re.search(r"(\w+)\s*$", q).group(1) for q in params.split(",")]


class Recorder(object):
    """stands in for the bound library: records (name, arguments), a pointer as its address, and returns 0 or ``returns[name]``"""

    def __init__(self, returns=None):
        self.calls, self.returns = [], returns or {}

    def __getattr__(self, name):
        def call(*args):
            self.calls.append((name, [a.value if isinstance(a, ctypes.c_void_p) else a for a in args]))
            return self.returns.get(name, 0)
        return call


def _expect(rec, name, **by_name):
    assert [c[0] for c in rec.calls] == [name], rec.calls
    args = rec.calls[0][1]
    assert list(by_name) == _params(name) and len(args) == len(by_name), (name, len(args))
    for (pname, want), got in zip(by_name.items(), args):
        assert got == want and type(got) is type(want), (name, pname, got, want)


def test_launchers_pass_every_parameter_by_its_header_name():
    from allrank_amd import _lib, saving as S
    st = ctypes.c_void_p(0x5EED)
    X = torch.zeros((7, 16), dtype=torch.float32)[:, :12]                       # 7 rows, 12 columns, row stride 16
    y, qid = torch.zeros(7), torch.zeros(7, dtype=torch.int64)
    lb, bad, text = torch.zeros(7, dtype=torch.int64), torch.zeros(1, dtype=torch.int32), torch.zeros(333, dtype=torch.uint8)
    rec = Recorder()
    S.libsvm_line_bytes(rec, st, X, y, qid, -1.0, 1, lb, bad)
    _expect(rec, "ltrx_libsvm_line_bytes", X=X.data_ptr(), ldx=16, y=y.data_ptr(), qid=qid.data_ptr(), n_rows=7, F=12, pad_value=-1.0,
            index_base=1, line_bytes=lb.data_ptr(), bad=bad.data_ptr(), stream=st.value)
    rec = Recorder()
    S.libsvm_format(rec, st, X, y, qid, -1.0, 0, lb, text)
    _expect(rec, "ltrx_libsvm_format", X=X.data_ptr(), ldx=16, y=y.data_ptr(), qid=qid.data_ptr(), n_rows=7, F=12, pad_value=-1.0,
            index_base=0, line_start=lb.data_ptr(), n_bytes=333, text=text.data_ptr(), stream=st.value)
    with pytest.raises(RuntimeError, match=r"libsvm_format failed: invalid argument"):
        S.libsvm_format(Recorder(returns={"ltrx_libsvm_format": -1}), st, X, y, qid, -1.0, 0, lb, text)
    for name in ("ltrx_libsvm_line_bytes", "ltrx_libsvm_format"):
        assert _lib.PROTOTYPES[name][0] == "int" and _lib.PROTOTYPES[name][1][-1] == "ltrx_stream_t"
        assert len(_lib.SIGNATURES[name][1]) == len(_params(name))
    assert _lib.PROTOTYPES["ltrx_debug_format_g16"] == ("int", ["*", "int64_t", "*", "*"])               # host-only: no stream


def test_each_writer_call_is_written_once_in_saving_py():
    import ast
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    names, seen = ("ltrx_libsvm_line_bytes", "ltrx_libsvm_format", "ltrx_debug_format_g16"), {}
    for dirpath, _, files in os.walk(os.path.join(root, "allrank_amd")):
        for f in files:
            if f.endswith(".py"):
                path = os.path.join(dirpath, f)
                for node in ast.walk(ast.parse(open(path).read(), path)):
                    if isinstance(node, ast.Call) and isinstance(node.func, ast.Attribute) and node.func.attr in names:
                        seen.setdefault(node.func.attr, []).append(os.path.relpath(path, root))
    assert seen == {name: [os.path.join("allrank_amd", "saving.py")] for name in names[:2]}, seen


# ---- the fixture's drift guard ---------------------------------------------------------------------------------------------
@pytest.mark.skipif(not reference_available(), reason="needs a checkout of allegro/allRank (ALLRANK_REFERENCE)")
def test_committed_fixture_equals_the_live_reference(golden):
    built = G.build()
    assert list(built) == ["svmwrite_golden.npz"]
    fresh = built["svmwrite_golden.npz"]
    assert set(fresh) == set(golden)
    for k, v in fresh.items():
        a, b = np.asarray(golden[k]), np.asarray(v)
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), k          # exactly: -0.0 and all
