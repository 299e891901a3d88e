"""-m gpu: libsvm text written on the device (allrank_amd/saving.py, allrank_amd/csrc/ltrx_svmwrite.hip, ltrx_fmt.h).  Every comparison
is byte for byte: with the reference's own files (tests/golden/svmwrite_golden.npz), with text built here by Python's ``%.16g``, or
with what the device parser reads back.  Not covered: a text above 2 GiB in one chunk (offsets are int64 by contract; a test that
large does not belong in the suite)."""
import os

import numpy as np
import pytest
import torch

from tests.golden import make_golden_svmwrite as G

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "svmwrite_golden.npz")


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def _python_text(X, y, qid, index_base=0):
    """the lines of the kept rows as Python prints them (X, y fp32 numpy)"""
    lines = []
    for r in range(X.shape[0]):
        row = X[r].tolist()
        feats = " ".join("%d:%.16g" % (f + index_base, v) for f, v in enumerate(row) if v != 0)
        lines.append("%.16g qid:%d %s\n" % (float(y[r]), qid[r], feats))
    return "".join(lines).encode("ascii")


@pytest.mark.parametrize("source", ["cpu", "device"])
@pytest.mark.parametrize("F", G.FS)
def test_device_path_writes_the_references_bytes(golden, tmp_path, F, source):
    from allrank_amd import saving as S
    x, y, want = golden["F%d.x" % F], golden["F%d.y" % F], golden["F%d.text" % F].tobytes()
    X, Y = G.slate_list(x, y, golden["lens"], golden["as_torch"])
    cube_x, cube_y = torch.from_numpy(x), torch.from_numpy(y)
    if source == "device":                                     # (numpy slates stay on the host: the list is mixed three ways)
        X, Y = ([v.to(DEV) if torch.is_tensor(v) else v for v in side] for side in (X, Y))
        cube_x, cube_y = cube_x.to(DEV), cube_y.to(DEV)
    path = tmp_path / "list.svm"
    S.write_to_libsvm_without_masked(str(path), X, Y)
    assert S.last_run == {"engine": "device", "reason": "", "rows": int((y != -1).sum()), "bytes": len(want)}
    assert path.read_bytes() == want
    S.write_slates(str(tmp_path / "cube.svm"), cube_x, cube_y)
    assert S.last_run["engine"] == "device" and (tmp_path / "cube.svm").read_bytes() == want
    assert sorted(p.name for p in tmp_path.iterdir()) == ["cube.svm", "list.svm"]


def test_random_bit_patterns_print_as_python_prints_them(tmp_path):
    """2^18 finite fp32 bit patterns as a [2048, 128] matrix and 2048 labels from the same draw: the device build of the formatter"""
    from allrank_amd import saving as S
    bits = np.random.default_rng(18).integers(0, 2 ** 32, 2048 * 129, dtype=np.uint64).astype(np.uint32)
    bits[(bits & 0x7F800000) == 0x7F800000] &= np.uint32(0xBFFFFFFF)      # an all-ones exponent loses a bit: finite
    v = bits.view(np.float32)
    assert np.isfinite(v).all() and (np.abs(v[v != 0]) < 1.17549435e-38).sum() > 100        # denormals are in the draw
    X, y = v[:2048 * 128].reshape(2048, 128), v[2048 * 128:].copy()
    y[y == -1.0] = -1.5                                                    # (-1 is the padding label)
    path = tmp_path / "sweep.svm"
    S.write_slates(str(path), X.reshape(2048, 1, 128), y.reshape(2048, 1))
    assert S.last_run["engine"] == "device" and S.last_run["rows"] == 2048
    got, want = path.read_bytes(), _python_text(X, y, np.arange(2048))
    if got != want:
        a, b = got.split(b"\n"), want.split(b"\n")
        first = next(i for i in range(min(len(a), len(b))) if a[i] != b[i])
        pytest.fail("line %d differs:\n%r\n%r" % (first, a[first][:300], b[first][:300]))


def test_the_bytes_do_not_depend_on_the_chunking(golden, tmp_path, monkeypatch):
    """one slate per chunk and two: at least 3 chunks, a chunk that is padding from end to end (slate 1), chunk boundaries inside the
    run of padded rows from the end of slate 0 to the end of slate 1"""
    from allrank_amd import saving as S
    F = max(G.FS)
    x, y, want = golden["F%d.x" % F], golden["F%d.y" % F], golden["F%d.text" % F].tobytes()
    assert (y[0, -3:] == -1).all() and (y[1] == -1).all() and (y[2, 0] != -1)
    slate_bytes = x.shape[1] * F * 4
    X, Y = G.slate_list(x, y, golden["lens"], golden["as_torch"])
    for chunk, least in ((slate_bytes, 11), (2 * slate_bytes + 1, 6), (1, 11)):
        monkeypatch.setattr(S, "CHUNK_BYTES", chunk)
        calls = []
        real = S.libsvm_line_bytes
        monkeypatch.setattr(S, "libsvm_line_bytes", lambda *a: (calls.append(1), real(*a))[1])
        S.write_slates(str(tmp_path / "cube.svm"), x, y)
        assert len(calls) == least >= 3 and (tmp_path / "cube.svm").read_bytes() == want, chunk
        S.write_to_libsvm_without_masked(str(tmp_path / "list.svm"), X, Y)
        assert len(calls) >= least + 3 and (tmp_path / "list.svm").read_bytes() == want, chunk
        monkeypatch.setattr(S, "libsvm_line_bytes", real)


def _round_trip_data(n=9, L=7, F=37, seed=5):
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((n, L, F)) * 10.0 ** rng.integers(-30, 31, (n, L, F))).astype(np.float32)
    x[rng.random(x.shape) < 0.4] = 0.0
    x[rng.random(x.shape) < 0.1] = -0.0
    y = rng.integers(0, 5, (n, L)).astype(np.float32) + np.float32(0.25) * rng.integers(0, 4, (n, L)).astype(np.float32)
    y[:, L - 2:] = -1.0
    y[4] = -1.0
    x[0, 0, 0], x[0, 0, F - 1] = 3.5, -1e-7                                  # the first and the last column are in the file
    return x, y


def test_round_trip_through_the_device_parser(tmp_path):
    from allrank_amd import saving as S
    from allrank_amd.data import parse_svm_file_on_device
    x, y = _round_trip_data()
    n, L, F = x.shape
    path = tmp_path / "rt.svm"
    S.write_slates(str(path), torch.from_numpy(x).to(DEV), torch.from_numpy(y).to(DEV), first_qid=7)
    X2, y2, q2 = (t.cpu().numpy() for t in parse_svm_file_on_device(str(path), DEV))
    keep = y.reshape(-1) != -1
    want_x = x.reshape(-1, F)[keep] + np.float32(0.0)                        # -0.0 arrives as +0.0
    assert not np.signbit(want_x[want_x == 0]).any()
    assert X2.shape == want_x.shape and X2.tobytes() == want_x.tobytes()
    assert y2.tobytes() == y.reshape(-1)[keep].tobytes()
    assert np.array_equal(q2, (7 + np.repeat(np.arange(n), L))[keep]) and q2.dtype == np.int64


def test_kernels_on_a_strided_matrix_write_inside_the_text_only():
    """the two launches themselves: rows 40 floats apart, one-based indices, a NaN pad (every row kept), the text at every alignment
    modulo 4 with sentinels before and behind it; and a line_start that points outside: nothing outside [0, n_bytes) is written"""
    from allrank_amd import _lib as LB, saving as S
    x, y = _round_trip_data(n=5, L=5, F=37, seed=6)
    x, y = x.reshape(-1, 37), y.reshape(-1)
    n = x.shape[0]
    qid = np.arange(n, dtype=np.int64) * 1000003 - 5
    wide = torch.full((n, 40), float("nan"), device=DEV)
    wide[:, :37] = torch.from_numpy(x).to(DEV)
    X, yd, qd = wide[:, :37], torch.from_numpy(y).to(DEV), torch.from_numpy(qid).to(DEV)
    lib, st = LB.lib(), LB.stream_of(X)
    lb = torch.full((n,), -7, dtype=torch.int64, device=DEV)
    bad = torch.zeros(1, dtype=torch.int32, device=DEV)
    S.libsvm_line_bytes(lib, st, X, yd, qd, float("nan"), 1, lb, bad)
    want = _python_text(x, y, qid, index_base=1)
    lines = [v + b"\n" for v in want.split(b"\n")[:-1]]
    assert lb.cpu().tolist() == [len(v) for v in lines] and int(bad.item()) == 0
    start = torch.cumsum(lb, 0) - lb
    total = len(want)
    for shift in range(4):
        buf = torch.full((64 + total + 64,), 0xAA, dtype=torch.uint8, device=DEV)
        text = buf[60 + shift:60 + shift + total]
        S.libsvm_format(lib, st, X, yd, qd, float("nan"), 1, start, text)
        got = buf.cpu().numpy()
        assert got[60 + shift:60 + shift + total].tobytes() == want, shift
        assert (got[:60 + shift] == 0xAA).all() and (got[60 + shift + total:] == 0xAA).all(), shift
    # offsets that do not belong to these rows: row 0 starts 50 bytes before the text, row 1 five bytes before its end, the others far
    # outside on either side.  What falls inside is written, nothing else.
    assert len(lines[0]) > 60 and len(lines[1]) > 5
    tail = len(lines[0]) - 50
    T = tail + 100
    buf = torch.full((64 + T + 64,), 0xAA, dtype=torch.uint8, device=DEV)
    wild = torch.tensor([-50, T - 5, 10 ** 12] + [-(10 ** 9), T] * ((n - 3) // 2), dtype=torch.int64, device=DEV)
    assert wild.numel() == n
    S.libsvm_format(lib, st, X, yd, qd, float("nan"), 1, wild, buf[64:64 + T])
    got = buf.cpu().numpy()
    assert (got[:64] == 0xAA).all() and (got[64 + T:] == 0xAA).all()
    assert got[64:64 + tail].tobytes() == lines[0][50:] and (got[64 + tail:64 + T - 5] == 0xAA).all()
    assert got[64 + T - 5:64 + T].tobytes() == lines[1][:5]


def test_clicked_slates_are_saved_as_the_host_path_saves_them(golden, tmp_path, monkeypatch):
    """rank_and_click.py:88 -> :92: what click_on_slates returns (device X slates, numpy click vectors) goes into the writer"""
    from allrank_amd import clicks as C, saving as S
    X, y = torch.from_numpy(golden["F20.x"]).to(DEV), torch.from_numpy(golden["F20.y"]).to(DEV)
    kept_X, clicks = C.click_on_slates((X, y), C.OnlyRelevant(2), include_empty=True)
    assert len(kept_X) == 11 and sum(int((c == 1).sum()) for c in clicks) > 10
    S.write_to_libsvm_without_masked(str(tmp_path / "device.svm"), kept_X, clicks)
    assert S.last_run["engine"] == "device" and S.last_run["rows"] == int((golden["F20.y"] != -1).sum())
    with monkeypatch.context() as m:
        m.setattr(torch.cuda, "is_available", lambda: False)
        S.write_to_libsvm_without_masked(str(tmp_path / "host.svm"), kept_X, clicks)
    assert S.last_run["engine"] == "host"
    got = (tmp_path / "device.svm").read_bytes()
    assert got == (tmp_path / "host.svm").read_bytes() and got.startswith(b"1 qid:0 ") and b" qid:10 " in got


def test_a_normalised_resident_set_is_saved_and_read_back():
    import json
    import tempfile
    from allrank_amd.data import DeviceSlates
    from allrank_amd.normalize import FeatureNormalizer
    from tests import featnorm_ref as R
    case = R.golden_case("b")
    with open(R.SETTINGS_WEB30K) as fh:
        settings = json.load(fh)
    slates = {r: DeviceSlates(case["roles"][r], case["y"][r], case["qid"][r], device=DEV) for r in R.ROLES}
    nz = FeatureNormalizer(**settings).fit(slates["train"], others=(slates["test"], slates["vali"]), roles=R.ROLES)
    with tempfile.TemporaryDirectory() as d:
        for r in R.ROLES:
            s = nz.apply(slates[r])
            assert np.array_equal(s.slate_qids.numpy(), case["qid"][r][s.offsets[:-1].cpu().numpy()]) and s.slate_qids.dtype == torch.int64
            x = s.x_items.cpu().numpy()
            assert (x[:, 0] != 0).any() and (x[:, -1] != 0).any() and not np.signbit(x[x == 0]).any()      # what a reader needs
            path = os.path.join(d, r + ".txt")
            s.write_svm_file(path)
            back = DeviceSlates.from_svm_file(path, DEV)
            assert back.x_items.cpu().numpy().tobytes() == x.tobytes(), r
            assert torch.equal(back.y_items, s.y_items) and torch.equal(back.offsets, s.offsets), r
            assert torch.equal(back.slate_qids, s.slate_qids), r
            s.write_svm_file(path, zero_based=False)                          # one-based: every index one higher, the same values
            again = DeviceSlates.from_svm_file(path, DEV)
            assert torch.equal(again.x_items, s.x_items) and torch.equal(again.slate_qids, s.slate_qids), r
            with open(path, "rb") as fh:
                assert b" 0:" not in fh.read()


def test_a_nan_in_a_kept_row_is_refused_and_leaves_no_file(tmp_path):
    from allrank_amd import saving as S
    x = torch.ones((3, 4, 6), device=DEV)
    y = torch.tensor([[1.0, 0.0, -1.0, -1.0]] * 3, device=DEV)
    path = tmp_path / "out.svm"
    for where, what in (((1, 1, 5), float("nan")), ((2, 0, 0), float("inf"))):
        bad = x.clone()
        bad[where] = what
        with pytest.raises(ValueError, match="NaN or an infinity"):
            S.write_slates(str(path), bad, y)
        assert list(tmp_path.iterdir()) == []
    ybad = y.clone()
    ybad[0, 1] = float("nan")
    with pytest.raises(ValueError, match="NaN or an infinity"):
        S.write_slates(str(path), x, ybad)
    with pytest.raises(ValueError, match="no row to write"):
        S.write_slates(str(path), x, torch.full_like(y, -1.0))
    assert list(tmp_path.iterdir()) == []
    bad = x.clone()
    bad[0, 2, 1], bad[2, 3, 3] = float("nan"), float("inf")                  # padded rows: not an error
    S.write_slates(str(path), bad, y)
    assert S.last_run["engine"] == "device" and path.read_bytes() == b"".join(
        b"%d qid:%d 0:1 1:1 2:1 3:1 4:1 5:1\n" % (lab, q) for q in range(3) for lab in (1, 0))
