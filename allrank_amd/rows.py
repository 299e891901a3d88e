"""The variable-length machinery of the fused step and the forward-only scorer: which rows a pass runs over, and how values move
between those rows and the padded [B, L] grid the loss kernels work on.

A forward-buffer set (``engine._alloc_forward``) has one of three row LAYOUTS:

  "grid"   the padded B * L rows, with a key-padding mask.  Nothing moves.
  "index"  the valid items packed through a host-sized index ``idx`` [n] (``FusedTrainer(compact=True)``): the row count is n
           rounded up to 32 and a launch argument, so the step runs eagerly; interior padding is accepted.
  "cu"     the valid items packed from ``cu_seqlens`` in device memory (``FusedTrainer(compact="graph")``, ``FusedScorer``): the
           row count is ``row_bucket(n, cap)`` and no launch argument depends on the batch, so a pass is captured per bucket; the
           valid items come first in every slate.

Here: the row ladder (``row_bucket``, ``set_rows``), the batch stager of the packed layouts (``_stage_host``, ``_Stager``), the
device count (``count_valid``: torch only, runs on CPU tensors too), the ONE staging of a "cu" buffer set (``stage_cu``) and the four
movers a pass makes -- each takes the buffer set ``bs`` and decides by ``bs.layout`` (and ``bs.saved``: a backward follows), each
launches through allrank_amd/kernels.py, none allocates or syncs (they are recorded into hipGraphs).
"""
import torch

from . import kernels as KN


def row_bucket(n, cap=None):
    """The rung of the scorer's row ladder that holds ``n`` packed rows: 32, 64, ..., 256, then steps of max(32, rung // 8 rounded
    down to a multiple of 32) -- every rung a multiple of 32, each at most 1/8 above the one below from 256 on, so a batch runs at
    most 31 rows (below 256) or 1/8 of its rows (above) of alignment padding.  ``cap`` (a multiple of 32): the largest rung."""
    b = 32
    while b < n:
        b += max(32, (b // 8) // 32 * 32)
    return b if cap is None else min(b, cap)


def set_rows(bs, n):
    """a "cu" buffer set runs ``n`` valid rows: its row bucket (alignment rows n .. rows-1: zero input, no slate, no gradient)"""
    bs.n_valid, bs.rows = n, row_bucket(max(n, 1), bs.cap)


def _stage_host(host, B, lengths, ids=None):
    """Pure host half of the stager: write ``[ids as int32 pairs, 2B |] cu_seqlens [B+1], stable longest-first order [B]`` of up to
    ``B`` slate ``lengths`` into the int32 buffer ``host`` (slates past the given ones: length 0, id 0); returns the valid-row count."""
    o = 2 * B if ids is not None else 0
    lens = torch.as_tensor(lengths, dtype=torch.int32).reshape(-1)
    full = torch.zeros(B, dtype=torch.int32)
    full[:lens.numel()] = lens
    host[o] = 0
    torch.cumsum(full, 0, dtype=torch.int32, out=host[o + 1:o + B + 1])
    host[o + B + 1:o + 2 * B + 1] = torch.argsort(full, descending=True, stable=True)
    if ids is not None:
        h64 = host[:o].view(torch.int64)
        h64.zero_()
        h64[:lens.numel()] = torch.as_tensor(ids, dtype=torch.int64).reshape(-1)
    return int(host[o + B])


class _Stager(object):
    """Device staging of one batch -- [slate ids (i64, as int32 pairs) |] cu_seqlens [B+1], launch order [B] in ONE tensor -- filled by
    one non-blocking upload from a ring of 4 pinned host buffers (a slot is reused after the copy that last used it has completed):
    only these few words cross PCIe per batch, and nothing syncs."""

    def __init__(self, dev, B, with_ids):
        self.B, o = B, 2 * B if with_ids else 0
        self.stage = torch.zeros(o + 2 * B + 1, dtype=torch.int32, device=dev)
        self.ids = self.stage[:o].view(torch.int64) if with_ids else None
        self.cu, self.order = self.stage[o:o + B + 1], self.stage[o + B + 1:]
        self._ring = [(torch.zeros(o + 2 * B + 1, dtype=torch.int32).pin_memory(), torch.cuda.Event()) for _ in range(4)]
        self._turn = 0

    def upload(self, lengths, ids=None):
        """``lengths`` (host or device ints, at most B, range-checked by the caller) and, if given, slate ``ids`` -> device; the row count"""
        host, ev = self._ring[self._turn % len(self._ring)]
        self._turn += 1
        ev.synchronize()
        if lengths.is_cuda:                                   # (a device tensor costs the sync the host lengths are meant to avoid)
            lengths = lengths.cpu()
        n = _stage_host(host if ids is not None else host[-(2 * self.B + 1):], self.B, lengths, ids)
        self.stage.copy_(host, non_blocking=True)
        ev.record()
        return n


def count_valid(valid, cu, order, want=("n",)):
    """The device half of the stager, torch only (CPU tensors too): ``valid`` [slates <= B, L] bool -> ``cu`` [B+1] (prefix sums of
    the valid items per slate; slates past the given ones: length 0) and ``order`` [B] (stable longest-first), written in place, as
    ``_stage_host`` writes them for the same lengths.  Returns, as 0-d int32 tensors that nothing has synced on yet, those of
      "n": valid items,  "max_len": the longest slate,  "prefix_ok": 1 where the valid items come first in every slate
    that ``want`` names, in its order."""
    B, (n_sl, L) = order.numel(), valid.shape
    cnt = valid.sum(1, dtype=torch.int32)
    if n_sl < B:
        cnt = torch.cat([cnt, cnt.new_zeros(B - n_sl)])
    cu[0] = 0
    torch.cumsum(cnt, 0, dtype=torch.int32, out=cu[1:])
    order.copy_(torch.argsort(cnt, descending=True, stable=True))
    get = {"n": lambda: cu[B],
           "max_len": cnt.max,
           "prefix_ok": lambda: (valid == (torch.arange(L, device=valid.device)[None, :] < cnt[:n_sl, None])).all().to(torch.int32)}
    return {k: get[k]() for k in want}


def stage_cu(bs, lib, st, xb, positions=None, lengths=None, ids=None, valid=None, want=("n",), check=None):
    """The staging of one batch into the "cu" buffer set ``bs``, outside any capture: cu_seqlens and the launch order, the row
    bucket, and the valid rows of the padded features ``xb`` [.., L, F] (and of the int64 ``positions``, where the model has a
    positional encoding) gathered by ltrx_gather_rows_cu, which also writes the packed-row index and zero-fills the alignment rows.
    Host ``lengths`` (int32, range-checked by the caller; with slate ``ids`` where the set stages them): one upload through the
    pinned ring, no sync.  Without them ``valid`` is counted on the device -- ONE sync, which reads the valid-row count and whatever
    else of ``count_valid`` the caller ``want``s.  ``check(got)`` sees what was read before anything is sized or gathered: where a
    caller refuses a batch.  Returns ``got`` ({"n": ...} and the wanted figures the device count gave)."""
    if lengths is not None:
        got = {"n": bs._stager.upload(lengths, ids)}
    else:
        figures = count_valid(valid, bs.cu, bs.order, want)
        got = dict(zip(figures, torch.stack(list(figures.values())).tolist()))       # (host sync: n picks the bucket)
    if check is not None:
        check(got)
    n = got["n"]
    set_rows(bs, n)
    KN.gather_rows_cu(lib, st, xb, bs.cu, bs.B, bs.L, xb.shape[-1], bs.rows, bs.x_in, bs.idx, "gather_rows_cu(x)")
    if positions is not None:                                 # int64 positions move as pairs of 32-bit words
        ib = positions.to(xb.device, torch.int64).contiguous()
        KN.gather_rows_cu(lib, st, ib, bs.cu, bs.B, bs.L, 2, bs.rows, bs.idx_rows, None, "gather_rows_cu(indices)")
        bs.idx_rows[n:bs.rows].fill_(-1)                      # alignment rows -> the padding position
    return got


# ---- the four movers of a pass over the buffer set ``bs`` (recorded into hipGraphs: launches only) ---------------------------
def scores_to_grid(bs, lib, st, sc_rows, cols):
    """the scores of the packed rows -> the padded grid ``bs.scores_raw`` of the loss kernels, 0 on padded slots"""
    if bs.layout == "cu":                                     # padding 0, count from cu[B]
        KN.scatter_rows_cu(lib, st, sc_rows, bs.cu, bs.B, bs.L, cols, bs.rows, bs.scores_raw)
    elif bs.layout == "index":
        bs.scores_raw.zero_()
        KN.scatter_rows(lib, st, sc_rows, bs.idx, bs.n_valid, cols, bs.scores_raw)


def zero_attention_tail(bs, lib, st, o):
    """The attention wrote rows of slates only; the out-projection reads every row, and where a backward follows so does its weight
    gradient: the alignment rows of ``o`` are 0 there, whatever the buffer held -- the count read from cu[B] on the device"""
    if bs.layout == "cu" and bs.saved:
        KN.zero_rows_cu(lib, st, o, bs.cu, bs.B, bs.rows)


def grid_to_rows(bs, lib, st, dsc, cols):
    """d loss / d scores on the padded grid -> the rows of the pass (alignment rows: 0); the tensor the backward reads"""
    if bs.layout == "cu":
        KN.gather_rows_cu(lib, st, dsc, bs.cu, bs.B, bs.L, cols, bs.rows, bs.dsc_c, None, "gather_rows_cu(d scores)")
    elif bs.layout == "index":
        KN.gather_rows(lib, st, dsc, bs.idx, bs.n_valid, bs.rows, cols, bs.dsc_c)
    else:
        return dsc
    return bs.dsc_c


def zero_gradient_tail(bs, lib, st, dqkv):
    """alignment rows belong to no slate: no gradient leaves the attention backward there"""
    if bs.layout == "cu":
        KN.zero_rows_cu(lib, st, dqkv, bs.cu, bs.B, bs.rows)
    elif bs.layout == "index" and bs.rows > bs.n_valid:
        dqkv[bs.n_valid:bs.rows].zero_()
