"""Slates saved as libsvm / SVMlight text -- the third stage of the reference's second entry point (rank_and_click.py:92:
``write_to_libsvm_without_masked`` -> np.vstack -> scikit-learn's ``dump_svmlight_file``, about 2 M values/s on the host), written on
the device, byte for byte the file the reference writes.

    write_slates(path, X, y, first_qid=0)            # X [N, L, F], y [N, L], -1 on padding; slate s gets qid first_qid + s
    write_to_libsvm_without_masked(path, X, y)       # the reference's signature: iterables of per-slate [L_i, F] / [L_i]
    DeviceSlates.write_svm_file(path)                # a resident set with its labels and original query ids (allrank_amd/data.py)

THE TEXT.  ``<%.16g of y> qid:<q> <index>:<%.16g of x> ...\\n`` per kept row: zero-based indices, zeros (of either sign) left out, a
row without a non-zero value ends ``qid:N \\n``; a padded row (y == -1) is dropped, and a slate without a kept row still uses up its
qid (dataset_saving.py:22-28).  ``%.16g`` of the fp32 value is exact: allrank_amd/csrc/ltrx_fmt.h.

CHUNKS.  Rows go to the device ``CHUNK_BYTES`` (256 MiB) of features at a time, at least one slate: upload, pass A
(``ltrx_libsvm_line_bytes``), ``torch.cumsum`` and ONE host synchronisation for the total, pass B (``ltrx_libsvm_format``), a copy into
a pinned host buffer, an append to the file.  The file's bytes do not depend on the chunking.  The text is written to a temporary
file beside ``path`` that takes its name at the end: a failed call leaves nothing at ``path``.

REFUSALS, as the reference's (check_array inside dump_svmlight_file): ``ValueError`` for a non-finite label or value in a kept row,
and where no row is kept at all.  A non-finite number in a padded row is nobody's business.

HOST PATH.  Without a GPU, with labels or values that fp32 does not hold exactly (the kernels format fp32), or with F == 0 the same
bytes come from a small formatter below -- Python's own ``%.16g``, no scikit-learn, not the reference's function.  (With F == 0 the
reference refuses the array; here every kept row is its head, ``<y> qid:<q> \\n``.)  ``last_run`` = {"engine": "device" | "host",
"reason": str, "rows": kept rows, "bytes": bytes written}.  Never an exception for that reason.

The two kernel calls (include/ltrx.h, "libsvm text written on the device") are stated once, below, in the form of
allrank_amd/kernels.py: one ``ltrx_*`` call on the tensors handed in, the library and the stream as arguments.
"""
import os

import numpy as np
import torch

from . import _lib as LB
from ._lib import check, ptr as P

__all__ = ["write_slates", "write_to_libsvm_without_masked", "write_rows", "last_run", "CHUNK_BYTES"]

last_run = {"engine": None, "reason": "", "rows": 0, "bytes": 0}
CHUNK_BYTES = 256 << 20          # feature bytes of one upload
PADDED_Y_VALUE = -1.0            # allrank/data/dataset_loading.py:13


# ---- the kernel calls --------------------------------------------------------------------------------------------------
def libsvm_line_bytes(lib, st, X, y, qid, pad_value, index_base, line_bytes, bad):
    """line_bytes[r] (int64) = the length of row r's line, 0 where y[r] == pad_value; bad[0] (int32, zeroed by the caller) += the kept
    rows that hold a non-finite number.  ``X``: a [rows, F] fp32 matrix or a column-slice view with its own row stride."""
    check(lib.ltrx_libsvm_line_bytes(P(X), X.stride(0), P(y), P(qid), X.shape[0], X.shape[1], float(pad_value), int(index_base),
                                     P(line_bytes), P(bad), st), "libsvm_line_bytes")


def libsvm_format(lib, st, X, y, qid, pad_value, index_base, line_start, text):
    """row r's line at text[line_start[r]:]; ``line_start`` = the exclusive prefix sum of ``line_bytes``, ``text``: uint8 of their sum"""
    check(lib.ltrx_libsvm_format(P(X), X.stride(0), P(y), P(qid), X.shape[0], X.shape[1], float(pad_value), int(index_base),
                                 P(line_start), text.numel(), P(text), st), "libsvm_format")


# ---- engines: (X [n, F], y [n], qid [n]) -> the chunk's text ------------------------------------------------------------------
def _refuse(what):
    raise ValueError("allrank_amd.saving: %s" % what)


class _Device(object):
    """formats chunks on ``dev``; the pinned buffer is kept from chunk to chunk and grows when it must"""
    name = "device"

    def __init__(self, dev):
        self.dev, self.pinned = dev, None

    def text(self, X, y, qid, pad, index_base):
        """(the chunk's text as a uint8 numpy view of the pinned buffer -- valid until the next call --, rows kept)"""
        dev = self.dev
        X = X.to(dev, torch.float32)
        if X.stride(1) != 1:
            X = X.contiguous()
        y = y.to(dev, torch.float32).contiguous()
        qid = qid.to(dev, torch.int64).contiguous()
        lib, st = LB.lib(), LB.launch_stream(dev)
        n = int(X.shape[0])
        line_bytes = torch.empty(n, dtype=torch.int64, device=dev)
        bad = torch.zeros(1, dtype=torch.int32, device=dev)
        libsvm_line_bytes(lib, st, X, y, qid, pad, index_base, line_bytes, bad)
        end = torch.cumsum(line_bytes, 0)
        total, kept, nbad = (int(v) for v in torch.stack([end[-1], (line_bytes > 0).sum(), bad[0].to(torch.int64)]).cpu())   # the one sync
        if nbad:
            _refuse("%d row(s) to write hold a NaN or an infinity" % nbad)
        if total == 0:
            return np.empty(0, dtype=np.uint8), 0
        text = torch.empty(total, dtype=torch.uint8, device=dev)
        libsvm_format(lib, st, X, y, qid, pad, index_base, end - line_bytes, text)
        if self.pinned is None or self.pinned.numel() < total:
            self.pinned = torch.empty(max(total, 1 << 20), dtype=torch.uint8, pin_memory=True)
        self.pinned[:total].copy_(text)                        # (a copy to pinned memory returns once it is done)
        torch.cuda.current_stream(dev).synchronize()
        return self.pinned[:total].numpy(), kept


def _g16(v):
    return "%.16g" % v


class _Host(object):
    name = "host"

    def text(self, X, y, qid, pad, index_base):
        def host(v):
            if not torch.is_tensor(v):
                return np.asarray(v)
            v = v.detach().cpu()
            return (v.float() if v.dtype in (torch.float16, torch.bfloat16) else v).numpy()      # (numpy has no bfloat16; fp32 holds both)
        X, y, qid = host(X), host(y), host(qid)
        keep = np.flatnonzero(y != pad) if pad == pad else np.arange(y.shape[0])
        X, y, qid = X[keep], y[keep], qid[keep]
        if not (np.isfinite(X.astype(np.float64)).all() and np.isfinite(y.astype(np.float64)).all()):
            _refuse("row(s) to write hold a NaN or an infinity")
        label = (lambda v: "%d" % v) if y.dtype.kind in "iub" else (lambda v: _g16(float(v)))
        value = (lambda v: "%d" % v) if X.dtype.kind in "iub" else (lambda v: _g16(float(v)))
        lines = []
        for r in range(X.shape[0]):
            row = X[r]
            nz = np.flatnonzero(row != 0)
            lines.append("%s qid:%d %s\n" % (label(y[r]), qid[r], " ".join("%d:%s" % (f + index_base, value(row[f])) for f in nz)))
        return np.frombuffer("".join(lines).encode("ascii"), dtype=np.uint8), int(X.shape[0])


def _exact_in_fp32(t):
    """does fp32 hold every entry of the tensor / array ``t`` as it is?"""
    t = t if torch.is_tensor(t) else torch.as_tensor(np.asarray(t))
    if t.dtype in (torch.float32, torch.float16, torch.bfloat16, torch.uint8, torch.int8, torch.int16, torch.bool) or t.numel() == 0:
        return True
    if t.dtype.is_floating_point:
        back = t.to(torch.float32).to(t.dtype)
        return bool(((back == t) | (t != t)).all())                  # (a NaN is refused later, by either engine)
    return bool((t.abs() <= (1 << 24)).all())


def _engine(F, arrays):
    """the engine for a call over ``arrays`` (every X and y of it) and the reason where that is the host's"""
    why = ""
    if not torch.cuda.is_available():
        why = "no GPU"
    elif not os.path.exists(LB.LIB_PATH):
        why = "libltrx.so is not built"
    elif F == 0:
        why = "no feature columns (F == 0)"
    elif not all(_exact_in_fp32(a) for a in arrays):
        why = "labels or values that fp32 does not hold exactly"
    if why:
        return _Host(), why
    dev = next((a.device for a in arrays if torch.is_tensor(a) and a.is_cuda), None)
    return _Device(dev if dev is not None else torch.device("cuda", torch.cuda.current_device())), ""


def write_rows(path, chunks, engine, reason="", pad_value=PADDED_Y_VALUE, index_base=0):
    """the machinery under every writer: ``chunks`` yields (X [n, F], y [n], qid [n]) tensors or arrays, n > 0; their text goes to a
    temporary file beside ``path``, which takes its name once every chunk is written.  Fills ``last_run``."""
    path = os.fspath(path)
    tmp = "%s.tmp.%d" % (path, os.getpid())
    rows = nbytes = 0
    try:
        with open(tmp, "wb") as fh:
            for X, y, qid in chunks:
                text, kept = engine.text(X, y, qid, pad_value, index_base)
                fh.write(memoryview(text))
                rows, nbytes = rows + kept, nbytes + int(text.shape[0])
        if rows == 0:
            _refuse("no row to write (every row is padding)")
        os.replace(tmp, path)
    finally:
        if os.path.exists(tmp):
            os.remove(tmp)
    last_run.update(engine=engine.name, reason=reason, rows=rows, bytes=nbytes)


def _tensor(v):
    return v if torch.is_tensor(v) else torch.as_tensor(np.asarray(v))


def write_slates(path, X, y, first_qid=0):
    """X [N, L, F] and y [N, L] (CPU or device tensors, or arrays; -1 on padding) as libsvm text at ``path``: slate s is query
    ``first_qid + s``, padded rows are dropped."""
    X, y = _tensor(X), _tensor(y)
    if X.dim() != 3 or y.dim() != 2 or X.shape[:2] != y.shape:
        _refuse("write_slates takes X [N, L, F] and y [N, L], got %s and %s" % (tuple(X.shape), tuple(y.shape)))
    N, L, F = (int(v) for v in X.shape)
    if N * L == 0:
        _refuse("no row to write (X is %s)" % (tuple(X.shape),))
    engine, why = _engine(F, (X, y))
    per = max(1, int(CHUNK_BYTES // max(1, L * F * 4)))

    def chunks():
        for a in range(0, N, per):
            b = min(a + per, N)
            yield X[a:b].reshape((b - a) * L, F), y[a:b].reshape(-1), torch.arange(first_qid + a, first_qid + b, dtype=torch.int64).repeat_interleave(L)
    write_rows(path, chunks(), engine, why)


def write_to_libsvm_without_masked(path, X, y):
    """
    This function writes given X's and y's in svmlight / libsvm file format.
    It supports padded documents - they are removed from the written dataset.
    Slates are identified by a 'qid' column within the file.
    (allrank/data/dataset_saving.py:9-32)

    :param path: a path to save libsvm file
    :param X: Iterable of lists of document vectors ([L_i, F] arrays or tensors, CPU or device, mixed; lengths may differ)
    :param y: Iterable of lists of document relevancies ([L_i])
    """
    pairs = [(_tensor(a), _tensor(b)) for a, b in zip(X, y)]
    if not pairs:
        _refuse("no row to write (no slates)")
    for a, b in pairs:
        if a.dim() != 2 or b.dim() != 1 or a.shape[0] != b.shape[0] or a.shape[1] != pairs[0][0].shape[1]:
            _refuse("slates must be [L_i, F] / [L_i] pairs of one F, got %s and %s" % (tuple(a.shape), tuple(b.shape)))
    F = int(pairs[0][0].shape[1])
    engine, why = _engine(F, [t for pair in pairs for t in pair])
    home = engine.dev if isinstance(engine, _Device) else torch.device("cpu")

    def chunks():
        a = 0
        while a < len(pairs):
            b, held = a, 0
            while b < len(pairs) and (b == a or held + pairs[b][0].numel() * 4 <= CHUNK_BYTES):
                held += pairs[b][0].numel() * 4
                b += 1
            lens = torch.tensor([int(p[1].shape[0]) for p in pairs[a:b]], dtype=torch.int64)
            if int(lens.sum()) > 0:
                xs, ys = (torch.cat([p[k].to(home) for p in pairs[a:b]]) for k in (0, 1))       # (dtypes promote, as np.vstack's)
                yield xs, ys, torch.arange(a, b, dtype=torch.int64).repeat_interleave(lens)
            a = b
    write_rows(path, chunks(), engine, why)
