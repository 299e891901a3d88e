"""Device-resident learning-to-rank dataset with on-device FixLength -- SURVEY.md §8(f) row 1.

The reference loader (allrank/data/dataset_loading.py) keeps one numpy array per query on the host, pads / samples each
slate in Python inside DataLoader workers (FixLength, :32-93) and ships every batch over PCIe from pageable memory
(train_utils.py:95).  That tops out orders of magnitude below what the training step consumes.  Here the whole
dataset lives in HBM in CSR form (WEB30K fold 1: 2.27 M items x 136 fp32 = 1.2 GB of the 288 GB):

    x_items [n_items, F] f32,  y_items [n_items] f32,  offsets [n_slates + 1] i64,  item_of [n_slates, max_len] i64 (-1 = none)

and a batch is produced on the device by two HIP kernels (``ltrx_fixlength_positions`` + ``ltrx_assemble_batch``,
allrank_amd/csrc/ltrx_data.hip; no host round trip, no per-slate Python; ``_positions_torch`` is the same transform in torch
device ops, kept as the independent implementation the tests compare the kernel with):
  * slates shorter than ``slate_length`` are padded: features 0, label -1, index -1 (FixLength._pad, :81-93);
  * longer slates are subsampled WITHOUT replacement in random order (FixLength._sample, :61-79) by drawing one
    uniform key per item and keeping the top ``slate_length`` keys;
  * the reference's relevance rule is kept: if the sample contains no relevant item but the slate has some, then --
    exactly one relevant document in the slate: it replaces the last sampled slot (:72-74); otherwise the slate is
    re-sampled until a relevant item is in (:75-76).
Output per batch: ``(xb f32[B, L, F], yb f32[B, L], indices i64[B, L])`` exactly like ToTensor (:19-29), on the device.
The libsvm text itself is parsed on the device too (``parse_svm_file_on_device`` -> ``ltrx_libsvm_parse``: the file's bytes are
uploaded once, one thread per line; scikit-learn's load_svmlight_file, the reference's parser (:130), stays available as
``from_svm_file(..., parser="sklearn")`` and is what the parity test compares with).

Round 6 -- behind the plugin boundary: ``load_libsvm_dataset`` / ``load_libsvm_dataset_role`` / ``create_data_loaders`` below have the
signatures of allrank/data/dataset_loading.py:197-248 and are what ``allrank_amd.install()`` binds to those names (and to
``allrank.main``'s copies, main.py:8), so an unmodified main.py trains from HBM: ``DeviceLibSVMDataset`` (a ``DeviceSlates`` plus the
slate length of its role) and ``DeviceLoader`` (batch order drawn from torch's global generator exactly as the reference's
``DataLoader(shuffle=True)`` draws it -- same seeds, same slates per batch; under a process group a rank assembles ONLY its
contiguous block of each global batch: no full-batch collation, no host-to-device copy at all).

``sampling="reference"`` (opt-in; ALLRANK_AMD_SAMPLING=reference under main.py): the sampling branch is drawn on the HOST with the
reference's own numpy calls from the reference's own generator stream (``reference_picks``; labels of the long slates only, no
features), a few KB of picks are uploaded per batch and ``ltrx_assemble_batch_picked`` gathers the batch in one launch -- the same
items, ``indices`` and generator states as the reference's loader, for ``num_workers`` 0 and >= 1.
"""
import logging

import numpy as np
import torch

log = logging.getLogger("allrank_amd.data")

PADDED_Y_VALUE = -1
PADDED_INDEX_VALUE = -1
SAMPLING_MODES = ("device", "reference")


def sampling_mode(value=None):
    """the sampling mode named by ``value`` or, without one, by the environment variable ALLRANK_AMD_SAMPLING (default "device")"""
    import os
    mode = (value if value is not None else os.environ.get("ALLRANK_AMD_SAMPLING") or "device")
    mode = str(mode).lower()
    if mode not in SAMPLING_MODES:
        raise ValueError("allrank_amd.data: sampling must be 'device' or 'reference', got %r" % (mode,))
    return mode


def reference_picks(y, L, rng):
    """The L positions FixLength._sample (dataset_loading.py:61-79) picks from a slate with labels ``y`` (len(y) >= L), drawn from
    ``rng`` -- the numpy module (its global generator) or a RandomState -- with the reference's calls in the reference's order:
    choice without replacement (:70); no relevant item sampled -> the slate's only relevant item replaces a re-drawn last slot
    (:72-74), or, with other relevance in the slate, the draw is repeated (:75-76)."""
    n = len(y)
    while True:
        pick = rng.choice(n, L, replace=False)
        if y[pick].sum() == 0:
            total = y.sum()
            if total == 1:
                pick = np.concatenate([rng.choice(pick, L - 1, replace=False), [np.argmax(y)]])
            elif total > 0:
                continue
        return pick


def parse_svm_file_on_device(path, device="cuda", n_features=None):
    """(X f32[n, F], y f32[n], qid i64[n]) as device tensors, parsed on the GPU.  Feature indices follow scikit-learn's
    zero_based="auto": one-based unless the smallest index in the file is 0."""
    from . import _lib as LB
    lib = LB.lib()
    dev = torch.device(device)
    raw = np.fromfile(path, dtype=np.uint8)
    if raw.size == 0:
        raise ValueError("empty file: %s" % path)
    text = torch.from_numpy(raw).to(dev)
    nl = torch.nonzero(text == 10).flatten()
    starts = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), nl + 1])
    starts = starts[starts < text.numel()]
    # drop blank / comment-only lines like sklearn does
    first = text[starts]
    starts = starts[(first != 10) & (first != 13) & (first != 35)].contiguous()
    n = int(starts.numel())
    y = torch.empty(n, dtype=torch.float32, device=dev)
    qid = torch.empty(n, dtype=torch.int64, device=dev)
    mm = torch.tensor([2 ** 31 - 1, -1], dtype=torch.int32, device=dev)
    bad = torch.zeros(1, dtype=torch.int32, device=dev)
    st = LB.stream_of(text)
    LB.check(lib.ltrx_libsvm_parse(LB.ptr(text), LB.ptr(starts), n, int(text.numel()), LB.ptr(y), LB.ptr(qid), None, 0, 0, LB.ptr(mm),
                                   LB.ptr(bad), st), "libsvm_parse(scan)")
    lo, hi = (int(v) for v in mm.cpu())
    if int(bad.item()):
        raise ValueError("%d malformed line(s) in %s" % (int(bad.item()), path))
    base = 0 if lo == 0 else 1
    F = int(n_features) if n_features is not None else hi - base + 1
    X = torch.zeros((n, F), dtype=torch.float32, device=dev)
    LB.check(lib.ltrx_libsvm_parse(LB.ptr(text), LB.ptr(starts), n, int(text.numel()), None, None, LB.ptr(X), F, base, None, LB.ptr(bad),
                                   st), "libsvm_parse(fill)")
    return X, y, qid


class DeviceSlates(object):
    def __init__(self, X, y, query_ids, device="cuda"):
        """X: [n_items, F] array (dense or scipy sparse), y: [n_items], query_ids: [n_items]; items of one query must be
        contiguous (as in libsvm LTR files); queries keep their order of first appearance (dataset_loading.py:109-113)."""
        if hasattr(X, "toarray"):
            X = X.toarray()
        self.device = torch.device(device)
        if torch.is_tensor(X):                       # already on the device (parse_svm_file_on_device): only the query ids go to the host
            q = query_ids.cpu().numpy() if torch.is_tensor(query_ids) else np.asarray(query_ids)
            Xt, yt = X.to(self.device, torch.float32).contiguous(), y.to(self.device, torch.float32).contiguous()
        else:
            X = np.ascontiguousarray(X, dtype=np.float32)
            y = np.asarray(y, dtype=np.float32)
            q = np.asarray(query_ids)
            Xt, yt = torch.from_numpy(X).to(self.device), torch.from_numpy(y).to(self.device)
        change = np.flatnonzero(q[1:] != q[:-1]) + 1
        starts = np.concatenate([[0], change]).astype(np.int64)
        offsets = np.concatenate([starts, [len(q)]]).astype(np.int64)
        lens = np.diff(offsets)
        self.n_slates = int(len(lens))
        self.n_features = int(X.shape[1])
        self.longest_query_length = int(lens.max())
        self.lengths_host = torch.from_numpy(lens.astype(np.int32))
        self.slate_qids = torch.from_numpy(q[starts].astype(np.int64))      # host: every slate's query id as the source gave it
        self.x_items = Xt
        self.y_items = yt
        self.offsets = torch.from_numpy(offsets).to(self.device)
        self.lengths = torch.from_numpy(lens).to(self.device)
        pos = torch.arange(self.longest_query_length, device=self.device)[None, :]
        item = self.offsets[:-1, None] + pos
        self.item_of = torch.where(pos < self.lengths[:, None], item, torch.full_like(item, -1))
        # per-slate relevance totals for the sampling rule
        ypad = torch.where(self.item_of >= 0, self.y_items[self.item_of.clamp(min=0)], torch.zeros((), device=self.device))
        self.label_sum = ypad.sum(1)
        self.argmax_pos = ypad.argmax(1)
        self._host_labels = {}                 # L -> {slate id: float64 labels} of the slates with >= L items (host_labels)

    @classmethod
    def from_svm_file(cls, path, device="cuda", parser="device"):
        """libsvm / SVMlight text -> DeviceSlates.  parser="device" (default on a GPU): the file's bytes are uploaded and parsed
        by ``ltrx_libsvm_parse`` (one thread per line); parser="sklearn": the reference's host parser (dataset_loading.py:130)."""
        if parser == "device" and torch.device(device).type == "cuda":
            X, y, qid = parse_svm_file_on_device(path, device)
            return cls(X, y, qid, device)
        from sklearn.datasets import load_svmlight_file
        X, y, qid = load_svmlight_file(path, query_id=True)
        return cls(X, y, qid, device)

    def write_svm_file(self, path, zero_based=True):
        """the resident items as libsvm text at ``path``, with their labels and original query ids (``slate_qids``), formatted on the
        device (allrank_amd/saving.py) -- so a set normalised in place (allrank_amd/normalize.py) is saved as the text
        reproducibility/normalize_features.py would have dumped: ``dump_svmlight_file(X, y, path, query_id=qid)``, zero-based indices.
        Every item is a row (labels of -1 included: nothing here is padding).
        The reference's own quirk, kept: a zero is not written, so with zero-based indices and a column 0 that is zero in EVERY row no
        index 0 appears in the file, and a reader that guesses the base (scikit-learn's ``zero_based="auto"``, the reference's
        loader, ``from_svm_file``) takes the file for one-based and shifts every index down by one.  ``zero_based=False`` writes
        one-based indices, which such a reader always gets right."""
        from . import saving as SV
        F, dev = self.n_features, self.device
        engine, why = SV._engine(F, (self.x_items, self.y_items))
        qid_items = self.slate_qids.to(dev).repeat_interleave(self.lengths)
        per = max(1, int(SV.CHUNK_BYTES // max(1, F * 4)))
        n = int(self.x_items.shape[0])
        chunks = ((self.x_items[a:a + per], self.y_items[a:a + per], qid_items[a:a + per]) for a in range(0, n, per))
        SV.write_rows(path, chunks, engine, why, pad_value=float("nan"), index_base=0 if zero_based else 1)

    def __len__(self):
        return self.n_slates

    @property
    def shape(self):
        return [self.n_slates, self.longest_query_length, self.n_features]

    # ------------------------------------------------------------------------------------------------------------
    def _positions_torch(self, slates, L, generator):
        """[B, L] positions inside each slate (-1 = padding) following FixLength -- torch device ops (reference implementation
        of the kernel for the tests)."""
        lens = self.lengths[slates]
        B = slates.numel()
        maxlen = self.longest_query_length
        pos = torch.arange(L, device=self.device)[None, :].expand(B, L)
        out = torch.where(pos < lens[:, None], pos, torch.full_like(pos, -1))          # the padding branch (len < L)
        # reference: sample_size < dim -> pad, else sample (a slate of exactly L items is "sampled" = randomly permuted)
        long_rows = torch.nonzero(lens >= L, as_tuple=False).flatten()
        if long_rows.numel():
            todo = long_rows
            for _ in range(64):
                ls = lens[todo]
                keys = torch.rand((todo.numel(), maxlen), device=self.device, generator=generator)
                keys = torch.where(torch.arange(maxlen, device=self.device)[None, :] < ls[:, None], keys, torch.full_like(keys, -1.0))
                samp = keys.topk(L, dim=1).indices                                          # random subset, random order
                ysamp = self.y_items[self.item_of[slates[todo]].gather(1, samp)]
                none_rel = ysamp.sum(1) == 0
                tot = self.label_sum[slates[todo]]
                one = none_rel & (tot == 1)                                                  # dataset_loading.py:72-74
                samp[one, L - 1] = self.argmax_pos[slates[todo]][one]
                retry = none_rel & (tot != 1) & (tot > 0)                                    # :75-76
                out[todo[~retry]] = samp[~retry]
                todo = todo[retry]
                if todo.numel() == 0:
                    break
            if todo.numel():                    # astronomically unlikely: keep the last draw
                out[todo] = samp[retry]
        return out

    def positions(self, slates, L, seed):
        """[B, L] positions inside each slate (-1 = padding): FixLength on the device (ltrx_fixlength_positions)."""
        from . import _lib as LB
        LB.require_device(self.y_items, slates)
        slates = slates.to(torch.int64).contiguous()
        B = int(slates.numel())
        pos = torch.empty((B, int(L)), dtype=torch.int64, device=self.device)
        LB.check(LB.lib().ltrx_fixlength_positions(LB.ptr(self.offsets), LB.ptr(self.y_items), LB.ptr(slates), B, int(L),
                                                   self.longest_query_length, int(seed) & 0xFFFFFFFFFFFFFFFF, LB.ptr(pos),
                                                   LB.stream_of(self.y_items)), "fixlength_positions")
        return pos

    def batch(self, slates, slate_length, generator=None, seed=None):
        """slates: i64[B] slate ids -> (xb [B,L,F], yb [B,L], indices [B,L]) on the device.  ``seed`` keys the sampling of the
        slates longer than ``slate_length`` (default: drawn from ``generator`` -- one host sync; ``batches`` draws one seed per
        epoch and counts batches instead)."""
        from . import _lib as LB
        LB.require_device(self.x_items)
        L = int(slate_length)
        if seed is None:
            seed = int(torch.randint(0, 2 ** 62, (1,), device=self.device, generator=generator).item())
        slates = slates.to(device=self.device, dtype=torch.int64).contiguous()
        B = int(slates.numel())
        if B == 0:                                   # (an empty block of a short last batch under a process group)
            return (torch.empty((0, L, self.n_features), dtype=torch.float32, device=self.device),
                    torch.empty((0, L), dtype=torch.float32, device=self.device), torch.empty((0, L), dtype=torch.int64, device=self.device))
        pos = self.positions(slates, L, seed)
        xb = torch.empty((B, L, self.n_features), dtype=torch.float32, device=self.device)
        yb = torch.empty((B, L), dtype=torch.float32, device=self.device)
        idx = torch.empty((B, L), dtype=torch.int64, device=self.device)
        LB.check(LB.lib().ltrx_assemble_batch(LB.ptr(self.x_items), LB.ptr(self.y_items), LB.ptr(self.offsets), LB.ptr(slates), LB.ptr(pos),
                                              B, L, self.n_features, LB.ptr(xb), LB.ptr(yb), LB.ptr(idx), LB.stream_of(xb)),
                 "assemble_batch")
        return xb, yb, idx

    def host_labels(self, L):
        """{slate id: labels as float64 (the reference's label dtype)} of the slates that take FixLength's sampling branch at slate
        length ``L`` (>= L items) -- all the host needs to make the reference's draws.  Built on first use per ``L``: one download."""
        L = int(L)
        if L not in self._host_labels:
            lens = self.lengths_host.numpy()
            ids = np.flatnonzero(lens >= L)
            out = {}
            if len(ids):
                ids_d = torch.from_numpy(ids).to(self.device)
                n = self.lengths[ids_d]
                pos = torch.arange(int(n.max()), device=self.device)[None, :]
                items = (self.offsets[ids_d][:, None] + pos)[pos < n[:, None]]           # the long slates' items, slate after slate
                flat = self.y_items[items].cpu().numpy().astype(np.float64)
                cuts = np.cumsum(lens[ids])[:-1]
                out = dict(zip(ids.tolist(), np.split(flat, cuts)))
            self._host_labels[L] = out
        return self._host_labels[L]

    def _picked_args(self, slates, pick_row, picks):
        slates = slates.to(device=self.device, dtype=torch.int64).contiguous()
        pick_row = pick_row.to(device=self.device, dtype=torch.int32).contiguous()
        if picks is not None and picks.numel() == 0:
            picks = None
        if picks is not None:
            picks = picks.to(device=self.device, dtype=torch.int32).contiguous()
        return slates, pick_row, picks

    def _empty_batch(self, L):
        return (torch.empty((0, L, self.n_features), dtype=torch.float32, device=self.device),
                torch.empty((0, L), dtype=torch.float32, device=self.device), torch.empty((0, L), dtype=torch.int64, device=self.device))

    def batch_picked(self, slates, slate_length, pick_row, picks=None):
        """slates: i64[B] slate ids, pick_row: i32[B], picks: i32[n, L] or None -> (xb [B,L,F], yb [B,L], indices [B,L]) in ONE launch
        (ltrx_assemble_batch_picked): row b takes the positions ``picks[pick_row[b]]``, or its stored order where ``pick_row[b]`` < 0."""
        from . import _lib as LB
        LB.require_device(self.x_items)
        L = int(slate_length)
        slates, pick_row, picks = self._picked_args(slates, pick_row, picks)
        B = int(slates.numel())
        if B == 0:
            return self._empty_batch(L)
        if int(pick_row.numel()) != B or (picks is not None and (picks.dim() != 2 or int(picks.shape[1]) != L)):
            raise ValueError("batch_picked: pick_row must have one entry per slate and picks must be [n, %d]" % L)
        xb = torch.empty((B, L, self.n_features), dtype=torch.float32, device=self.device)
        yb = torch.empty((B, L), dtype=torch.float32, device=self.device)
        idx = torch.empty((B, L), dtype=torch.int64, device=self.device)
        LB.check(LB.lib().ltrx_assemble_batch_picked(LB.ptr(self.x_items), LB.ptr(self.y_items), LB.ptr(self.offsets), LB.ptr(slates),
                                                     LB.ptr(pick_row), LB.ptr(picks), 0 if picks is None else int(picks.shape[0]), B, L,
                                                     self.n_features, LB.ptr(xb), LB.ptr(yb), LB.ptr(idx), LB.stream_of(xb)),
                 "assemble_batch_picked")
        return xb, yb, idx

    def batch_picked_torch(self, slates, slate_length, pick_row, picks=None):
        """the batch of ``batch_picked`` through torch ops (tests; the counterpart of ``batch_torch``)"""
        L = int(slate_length)
        slates, pick_row, picks = self._picked_args(slates, pick_row, picks)
        if slates.numel() == 0:
            return self._empty_batch(L)
        lens = self.lengths[slates][:, None]
        pos = torch.arange(L, device=self.device)[None, :].expand(slates.numel(), L)
        if picks is not None:
            known = (pick_row >= 0) & (pick_row < picks.shape[0])
            taken = picks[pick_row.long().clamp(0, picks.shape[0] - 1)].to(torch.int64)
            pos = torch.where(known[:, None], taken, torch.where(pick_row[:, None] < 0, pos, torch.full_like(pos, -1)))
        else:
            pos = torch.where(pick_row[:, None] < 0, pos, torch.full_like(pos, -1))
        valid = (pos >= 0) & (pos < lens)
        item = torch.where(valid, self.offsets[slates][:, None] + pos, torch.zeros_like(pos))
        xb = self.x_items[item] * valid[:, :, None]
        yb = torch.where(valid, self.y_items[item], torch.full((), float(PADDED_Y_VALUE), device=self.device))
        idx = torch.where(valid, pos, torch.full_like(pos, PADDED_INDEX_VALUE))
        return xb, yb, idx

    def batch_torch(self, slates, slate_length, generator=None):
        """the same batch through torch device ops (tests)"""
        L = int(slate_length)
        pos = self._positions_torch(slates, L, generator)
        valid = pos >= 0
        item = self.item_of[slates].gather(1, pos.clamp(min=0))
        item = torch.where(valid, item, torch.zeros_like(item))
        xb = self.x_items[item] * valid[:, :, None]
        yb = torch.where(valid, self.y_items[item], torch.full((), float(PADDED_Y_VALUE), device=self.device))
        idx = torch.where(valid, pos, torch.full_like(pos, PADDED_INDEX_VALUE))
        return xb, yb, idx

    def batches(self, batch_size, slate_length=None, shuffle=False, generator=None, drop_last=False):
        """epoch iterator (DataLoader(batch_size, shuffle) semantics, dataset_loading.py:245-246); ``slate_length=None``
        pads to the longest slate like the validation transform (:185-194)."""
        L = self.longest_query_length if slate_length is None else int(slate_length)
        order = (torch.randperm(self.n_slates, device=self.device, generator=generator) if shuffle
                 else torch.arange(self.n_slates, device=self.device))
        # one seed per epoch (one host sync), a counter per batch: sampling of long slates never syncs inside the epoch
        base = int(torch.randint(0, 2 ** 40, (1,), device=self.device, generator=generator).item()) if L < self.longest_query_length else 0
        for k, s in enumerate(range(0, self.n_slates, batch_size)):
            ids = order[s:s + batch_size]
            if drop_last and ids.numel() < batch_size:
                break
            yield self.batch(ids, L, seed=(base << 22) + k)


def evaluate(model, dataset, metrics, batch_size=512, slate_length=None):
    """epoch-level metrics (compute_metrics / metric_on_epoch, train_utils.py:32-56) in one no-grad pass over a
    DeviceSlates dataset: {"ndcg_5": value, ...}; ``metrics`` = {"ndcg": [5, 10, ...]} like config.metrics."""
    from . import metrics as EM
    out = {}
    was_training = model.training
    model.eval()
    with torch.no_grad():
        acc = {name: [] for name in metrics}
        for xb, yb, idx in dataset.batches(batch_size, slate_length):
            sc = model.score(xb, yb == PADDED_Y_VALUE, idx)
            for name, ats in metrics.items():
                acc[name].append(getattr(EM, name)(sc, yb, ats=ats))
        for name, ats in metrics.items():
            vals = torch.cat(acc[name]).mean(0).cpu().numpy()
            for at, v in zip(ats, vals):
                out["%s_%d" % (name, at)] = float(v)
    model.train(was_training)
    return out


# ---------------------------------------------------------------------------------------------------------------------
# The reference's loader interface on top of DeviceSlates (allrank/data/dataset_loading.py:96-248) -- what install() binds
# ---------------------------------------------------------------------------------------------------------------------
class ShardBatch(tuple):
    """``(xb, yb, indices)`` as a DeviceLoader yields it: a plain 3-tuple for every consumer that unpacks it (the reference's own
    ``fit`` included), plus what a sharded consumer needs to know about the GLOBAL batch it is a block of:
      ``global_slates``  slates in the whole global batch (the loss divisor of SURVEY 8e),
      ``offset``         first row of this block inside the global batch,
      ``order_tag``      a checksum of the global batch's slate ids (host integer; every rank must hold the same one),
      ``lengths``        valid items per slate of THIS block as a host int32 tensor (variable-length execution sizes its launches
                         from it without a device round trip)."""

    def __new__(cls, tensors, global_slates, offset, order_tag, lengths=None):
        self = super(ShardBatch, cls).__new__(cls, tensors)
        self.global_slates, self.offset, self.order_tag, self.lengths = int(global_slates), int(offset), int(order_tag), lengths
        return self


class SlateIds(object):
    """One batch of ``DeviceLoader.id_batches``: this rank's block of a global batch as slate ids of the resident set ``slates``
    (``ids``: host int64) with their host item counts (``lengths``, clamped to the slate length) -- plus ``global_slates``,
    ``offset`` and ``order_tag`` with the meaning they have in ``ShardBatch``."""

    def __init__(self, slates, ids, lengths, global_slates, offset, order_tag):
        self.slates, self.ids, self.lengths = slates, ids, lengths
        self.global_slates, self.offset, self.order_tag = int(global_slates), int(offset), int(order_tag)


class _SlateIds(torch.utils.data.Dataset):
    """dataset of the numbers 0 .. n-1: a torch DataLoader over it yields the slate ids of every batch, i.e. the sampler /
    batch-sampler behaviour of the reference's loader (dataset_loading.py:245-246) without touching any data"""

    def __init__(self, n):
        self.n = int(n)

    def __len__(self):
        return self.n

    def __getitem__(self, i):
        return int(i)


class DeviceLibSVMDataset(object):
    """What ``load_libsvm_dataset`` returns instead of a ``LibSVMDataset`` (dataset_loading.py:96-165): the slates of one role in
    HBM (``slates``: DeviceSlates) plus the length its batches are fixed to -- ``slate_length`` for the training role, the longest
    slate for every other role (:212-227).  ``shape`` / ``longest_query_length`` / ``len()`` / indexing keep the reference's meaning
    (main.py:63-64 reads ``shape[-1]``); an item is the transformed slate ``(x [L, F], y [L], indices [L])`` -- on the device."""

    def __init__(self, slates, slate_length=None, sampling="device"):
        self.slates = slates
        self.slate_length = int(slates.longest_query_length if slate_length is None else slate_length)
        self.sampling = sampling_mode(sampling)          # how ``ds[i]`` samples a long slate (DeviceLoader has its own switch)

    @classmethod
    def from_svm_file(cls, svm_file_path, slate_length=None, device="cuda", parser="device", sampling="device"):
        return cls(DeviceSlates.from_svm_file(svm_file_path, device=device, parser=parser), slate_length, sampling)

    def __len__(self):
        return self.slates.n_slates

    @property
    def longest_query_length(self):
        return self.slates.longest_query_length

    @property
    def shape(self):
        return self.slates.shape

    @property
    def samples(self):
        """True if FixLength's sampling branch can occur (some slate has at least ``slate_length`` items, :55-58)"""
        return self.slates.longest_query_length >= self.slate_length

    def __getitem__(self, idx):
        if self.sampling == "reference":                 # FixLength draws from numpy's global generator (dataset_loading.py:70)
            L, dev = self.slate_length, self.slates.device
            y = self.slates.host_labels(L).get(int(idx))
            picks = None if y is None else torch.from_numpy(reference_picks(y, L, np.random).astype(np.int32))[None, :]
            xb, yb, ib = self.slates.batch_picked(torch.tensor([int(idx)], device=dev), L,
                                                  torch.tensor([-1 if y is None else 0], dtype=torch.int32, device=dev), picks)
            return xb[0], yb[0], ib[0]
        xb, yb, ib = self.slates.batch(torch.tensor([int(idx)], device=self.slates.device), self.slate_length,
                                       seed=int(np.random.randint(0, 2 ** 31 - 1)) if self.samples else 0)
        return xb[0], yb[0], ib[0]


class DeviceLoader(object):
    """The iteration contract of the reference's ``DataLoader(ds, batch_size=total, shuffle=..., drop_last=False)``
    (dataset_loading.py:245-246) over a DeviceLibSVMDataset: yields ``(xb f32[B, L, F], yb f32[B, L], indices i64[B, L])`` --
    already on the device, assembled there by ``ltrx_fixlength_positions`` + ``ltrx_assemble_batch``.

    * Batch composition: the slate ids of every batch come from a torch ``DataLoader`` over the ids 0..n-1 with the same
      ``batch_size`` / ``shuffle``, so the draws from torch's GLOBAL generator (worker base seed, RandomSampler seed) and the
      resulting permutation are the reference loader's: under main.py:36-38's seeds epoch e visits the same slates in the same
      batches in the same order.  ``burn()`` consumes the draws of one iteration without running it (``allrank_amd.fit`` skips the
      reference's extra passes over the loaders, train_utils.py:99,107, and keeps the generator in step this way).
    * FixLength: the padding branch is exact.  The sampling branch (slates of >= L items, :61-79) depends on ``sampling``:
      - ``"device"`` (default): drawn on the device (``ltrx_fixlength_positions``), keyed by one seed per iteration -- taken from
        numpy's global generator, the generator the reference samples from (:70) -- and the slate id: the reference's distribution,
        not its items.  ``num_workers`` is ignored.
      - ``"reference"``: the reference's own draws, made on the host batch by batch as each batch is requested (labels only; a few
        KB of picks are uploaded per batch and ``ltrx_assemble_batch_picked`` assembles the batch in one launch): the same items,
        ``indices`` and generator states as the reference's ``DataLoader(num_workers=W)``.  ``W == 0``: item by item, in batch order,
        from numpy's global generator.  ``W >= 1``: batch k is made by worker k % W, whose numpy generator torch's worker loop
        seeded with ``_generate_state(base_seed, worker)``; numpy's global generator is not touched.  A non-training role is
        padded to its longest slate, so its longest slate(s) are "sampled" (permuted) too and consume draws in every pass.
        ``burn()`` and ``id_batches()`` leave both global generators where a full pass of the reference's loader leaves them
        (``W == 0``: the pass's numpy draws are made and discarded); ``id_batches()`` keeps the stored item order.
    * ``world`` > 1: this rank yields its contiguous block (``parallel.shard_slates``, the rule of DataParallel.scatter) of each
      global batch as a ``ShardBatch``; nothing of the other ranks' blocks is assembled.  ``batch_size`` stays the GLOBAL size.
      Under ``"reference"`` every rank makes the draws of the whole global batch (the generator stream is shared)."""

    def __init__(self, dataset, batch_size, shuffle=False, rank=0, world=1, sampling="device", num_workers=0):
        from torch.utils.data import DataLoader
        self.dataset, self.batch_size, self.shuffle = dataset, int(batch_size), bool(shuffle)
        self.rank, self.world = int(rank), max(1, int(world))
        self.drop_last = False
        self.sampling = sampling_mode(sampling)
        self.num_workers = max(0, int(num_workers)) if self.sampling == "reference" else 0
        self._ids = DataLoader(_SlateIds(len(dataset)), batch_size=self.batch_size, shuffle=self.shuffle, num_workers=0)
        self.sampler = self._ids.sampler

    slate_length = property(lambda self: self.dataset.slate_length)

    def __len__(self):
        return len(self._ids)

    def _pass(self):
        """start one pass: (slate ids of every global batch as host int64 tensors, the numpy generator that makes batch k's draws).
        All of the pass's draws from torch's global generator (worker base seed, RandomSampler seed) happen here, as in ``iter`` of
        the reference's loader."""
        it = iter(self._ids)
        chunks = [c.to(torch.int64) for c in it]
        if self.num_workers == 0:
            return chunks, lambda k: np.random
        from torch.utils.data._utils.worker import _generate_state
        workers = [np.random.RandomState(_generate_state(it._base_seed, w)) for w in range(self.num_workers)]
        return chunks, lambda k: workers[k % self.num_workers]

    def _draw(self, ids, rng, labels, keep=None):
        """the reference's draws for one global batch, item by item in batch order; ``keep`` = (a, b): also return (pick_row i32[b-a],
        picks i32[n, L]) of that block of rows"""
        L = self.dataset.slate_length
        rows, picks = [], []
        for j, s in enumerate(ids.tolist()):
            y = labels.get(s)
            pick = reference_picks(y, L, rng) if y is not None else None
            if keep is not None and keep[0] <= j < keep[1]:
                rows.append(-1 if pick is None else len(picks))
                if pick is not None:
                    picks.append(pick)
        if keep is None:
            return None
        return np.asarray(rows, dtype=np.int32), (np.stack(picks).astype(np.int32) if picks else np.zeros((0, L), dtype=np.int32))

    def burn(self):
        """consume what ONE iteration over the reference's loader draws from the global generators, without assembling a batch"""
        if self.sampling == "reference" and self.num_workers == 0 and self.dataset.samples:
            chunks, rng = self._pass()
            labels = self.dataset.slates.host_labels(self.dataset.slate_length)
            for k, c in enumerate(chunks):
                self._draw(c, rng(k), labels)
            return
        next(iter(self._ids), None)

    def batch_shape(self):
        """(global slates per batch, slate length, fraction of valid slots over the whole set) -- no batch is consumed"""
        s, L = self.dataset.slates, self.dataset.slate_length
        valid = float(s.lengths.clamp(max=L).double().sum().item()) / max(1.0, float(s.n_slates) * L)
        return self.batch_size, L, valid

    @property
    def packable(self):
        """True when no slate is longer than the loader's slate length -- every non-training role, which the reference pads to its
        longest slate (:212-227) -- i.e. only FixLength's padding branch changes the content of a batch (a slate of exactly
        ``slate_length`` items is permuted by the sampling branch; its items, labels and positions are the same)"""
        return self.dataset.slate_length >= self.dataset.longest_query_length

    def id_batches(self):
        """The batches of ``__iter__`` -- same generator draws, same slates, same rank blocks -- as ``SlateIds`` instead of assembled
        tensors: for a consumer that builds the packed batch itself (engine.FusedScorer.run_resident).  Slates keep their stored item
        order (the padding branch of FixLength)."""
        from .parallel import shard_slates
        ds, L = self.dataset, self.dataset.slate_length
        if self.sampling == "reference":
            chunks, rng = self._pass()
            labels = ds.slates.host_labels(L) if (ds.samples and self.num_workers == 0) else None
        else:
            chunks, labels = [c.to(torch.int64) for c in self._ids], None   # the epoch's draws from torch's global generator, as __iter__
            if ds.samples:
                np.random.randint(0, 2 ** 31 - 1)                          # ... and the sampling seed __iter__ draws from numpy's
        weights = torch.arange(1, self.batch_size + 1, dtype=torch.int64)
        for k, c in enumerate(chunks):
            n = int(c.numel())
            a, b = shard_slates(n, self.rank, self.world)
            if labels:
                self._draw(c, rng(k), labels)                              # made where __iter__ makes them, and discarded
            tag = int((c * weights[:n]).sum().item()) & 0x7FFFFFFFFFFF
            yield SlateIds(ds.slates, c[a:b], ds.slates.lengths_host[c[a:b]].clamp(max=L), n, a, tag)

    def _upload_picks(self, rows, picks):
        """(pick_row i32[B], picks i32[n, L] or None) on the device: one small copy per batch, from pinned memory on a GPU so that the
        host never waits for the step in flight"""
        dev = self.dataset.slates.device
        nb = int(rows.size)
        host = torch.empty(nb + int(picks.size), dtype=torch.int32, pin_memory=dev.type == "cuda")
        host[:nb] = torch.from_numpy(rows)
        host[nb:] = torch.from_numpy(picks.reshape(-1))
        buf = host.to(dev, non_blocking=True)
        return buf[:nb], (buf[nb:].view(picks.shape) if picks.size else None)

    def _iter_reference(self):
        from .parallel import shard_slates
        ds, L = self.dataset, self.dataset.slate_length
        chunks, rng = self._pass()
        if not chunks:
            return
        labels = ds.slates.host_labels(L) if ds.samples else {}
        order = torch.cat(chunks).to(ds.slates.device)                 # ONE small upload per epoch (8 B per slate)
        start = 0
        weights = torch.arange(1, self.batch_size + 1, dtype=torch.int64)
        for k, c in enumerate(chunks):
            n = int(c.numel())
            a, b = shard_slates(n, self.rank, self.world)
            rows, picks = self._draw(c, rng(k), labels, keep=(a, b))    # the whole global batch's draws; this rank's block kept
            pick_row, picks = self._upload_picks(rows, picks)
            xb, yb, ib = ds.slates.batch_picked(order[start + a:start + b], L, pick_row, picks)
            tag = int((c * weights[:n]).sum().item()) & 0x7FFFFFFFFFFF
            start += n
            yield ShardBatch((xb, yb, ib), n, a, tag, ds.slates.lengths_host[c[a:b]].clamp(max=L))

    def __iter__(self):
        from .parallel import shard_slates
        if self.sampling == "reference":
            yield from self._iter_reference()
            return
        ds, L = self.dataset, self.dataset.slate_length
        chunks = [c.to(torch.int64) for c in self._ids]                # host tensors; all of the epoch's generator draws happen here
        seed = int(np.random.randint(0, 2 ** 31 - 1)) if ds.samples else 0
        if not chunks:
            return
        order = torch.cat(chunks).to(ds.slates.device)                 # ONE small upload per epoch (8 B per slate)
        start = 0
        weights = torch.arange(1, self.batch_size + 1, dtype=torch.int64)
        for c in chunks:
            n = int(c.numel())
            a, b = shard_slates(n, self.rank, self.world)
            xb, yb, ib = ds.slates.batch(order[start + a:start + b], L, seed=seed)
            tag = int((c * weights[:n]).sum().item()) & 0x7FFFFFFFFFFF
            start += n
            yield ShardBatch((xb, yb, ib), n, a, tag, ds.slates.lengths_host[c[a:b]].clamp(max=L))


def _local_path(input_path, role):
    import os
    return os.path.join(input_path, "{}.txt".format(role))


def load_libsvm_role(input_path, role, device=None):
    """dataset_loading.py:168-182 (``{input_path}/{role}.txt`` -> dataset, no transform yet = padded to its longest slate): the
    file's bytes go to the GPU once and are parsed there.  ``ds[i]`` samples as ALLRANK_AMD_SAMPLING says."""
    from .launch import get_torch_device
    dev = torch.device(device) if device is not None else get_torch_device()
    path = _local_path(input_path, role)
    if str(input_path).startswith("gs://"):
        raise NotImplementedError("allrank_amd.data: %s is a GCS path -- copy the files to local storage (the device-resident loader "
                                  "reads local files; the reference's GCS helper, utils/file_utils.py, is out of scope)" % path)
    log.info("will load %s data from %s", role, path)
    ds = DeviceLibSVMDataset.from_svm_file(path, None, device=dev, sampling=sampling_mode())
    log.info("%s DS shape: %s (resident on %s)", role, ds.shape, dev)
    return ds


def load_libsvm_dataset_role(role, input_path, slate_length, device=None):
    """dataset_loading.py:212-227: the training role is fixed to ``slate_length``, every other role to its longest slate"""
    ds = load_libsvm_role(input_path, role, device)
    if role == "train":
        ds.slate_length = int(slate_length)
    else:
        log.info("Will pad to the longest slate: %d", ds.longest_query_length)
        ds.slate_length = int(ds.longest_query_length)
    return ds


NORMALIZE_ENV = "ALLRANK_AMD_NORMALIZE"
NORMALIZE_ROLES = ("train", "test", "vali")             # the files reproducibility/normalize_features.py reads (:31-33)


def _normalizer_from(settings):
    """the FeatureNormalizer ``settings`` names: one already built, or the path of a settings file"""
    from .normalize import FeatureNormalizer
    if isinstance(settings, FeatureNormalizer):
        return settings
    try:
        return FeatureNormalizer.from_settings(settings)
    except (OSError, ValueError) as e:
        raise type(e)("allrank_amd.data: cannot read the feature normalisation settings %r (%s, or load_libsvm_dataset's normalize=): %s"
                      % (settings, NORMALIZE_ENV, e))


def _normalize_loaded(nz, input_path, loaded, also=()):
    """Fit ``nz`` on the train role and apply it to every data set of ``loaded`` ({role: DeviceLibSVMDataset}) and of ``also`` (further
    copies of a loaded role).  The decision which columns are >= 0 is taken over train, test and vali as the reference script takes
    it -- over those of the three files that exist in ``input_path``: a role that was not loaded is parsed on the device, reduced to its
    per-column minimum and freed; a missing one is logged and left out of ``nz.roles``."""
    import os
    x_train = loaded["train"].slates.x_items
    roles, minima = [], []
    for role in NORMALIZE_ROLES + tuple(r for r in loaded if r not in NORMALIZE_ROLES):     # (a validation role of another name counts too)
        if role in loaded:
            minima.append(nz.minimum(loaded[role].slates.x_items))
        elif os.path.exists(_local_path(input_path, role)):
            log.info("feature normalisation: reading %s for the sign decision only", _local_path(input_path, role))
            X, _, _ = parse_svm_file_on_device(_local_path(input_path, role), x_train.device)
            minima.append(nz.minimum(X))
            del X
        else:
            log.warning("feature normalisation: %s is missing -- the decision which features take the logarithm is taken without the "
                        "%s role", _local_path(input_path, role), role)
            continue
        roles.append(role)
    nz.fit_with_minima(x_train, minima, roles)
    for ds in list(loaded.values()) + list(also):
        nz.apply(ds.slates)
        ds.normalizer = nz
    log.info("feature normalisation: statistics from %s, roles %s, %d of %d features take the logarithm, %d wanted it and hold negative "
             "values: %s", _local_path(input_path, "train"), roles, nz.report["log"], nz.n_features, len(nz.no_log_negative),
             nz.no_log_negative)


def load_libsvm_dataset(input_path, slate_length, validation_ds_role, device=None, normalize=None):
    """dataset_loading.py:197-209: (train, validation) datasets -- resident in HBM.  ``normalize`` (a settings file's path or a
    ``FeatureNormalizer``; default: the environment variable ALLRANK_AMD_NORMALIZE, which main.py's callers set) normalises the features
    of both on the device with statistics of ``train.txt`` (allrank_amd/normalize.py) and hangs the normaliser on them as
    ``ds.normalizer``; without it the data sets are what they always were."""
    import os
    settings = normalize if normalize is not None else (os.environ.get(NORMALIZE_ENV) or None)
    nz = _normalizer_from(settings) if settings is not None else None
    train = load_libsvm_dataset_role("train", input_path, slate_length, device)
    val = load_libsvm_dataset_role(validation_ds_role, input_path, slate_length, device)
    if nz is not None:
        if validation_ds_role == "train":                # two copies of one role: each is normalised once
            _normalize_loaded(nz, input_path, {"train": train}, also=(val,))
        else:
            _normalize_loaded(nz, input_path, {"train": train, validation_ds_role: val})
    return train, val


def processing_units():
    """(rank, world) of the slate sharding: the process group's when one is up (or the launcher's record of it), else one unit"""
    import torch.distributed as dist
    from . import launch
    if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
        return dist.get_rank(), dist.get_world_size()
    if launch.world_size() > 1:
        return launch.rank(), launch.world_size()
    return 0, 1


def create_data_loaders(train_ds, val_ds, num_workers, batch_size):
    """dataset_loading.py:230-248: train loader shuffled, validation loader not, drop_last False, both with ``units x batch_size``
    slates per GLOBAL batch (":240-241: multiplying the batch size by the processing units count").  The processing units are the
    ranks of the process group when one is up (one process per GPU, ``allrank_amd.launch``), else the visible GPUs as in the
    reference.  DeviceLibSVMDataset -> DeviceLoader; any other dataset -> the reference's torch DataLoader.  The environment variable
    ALLRANK_AMD_SAMPLING (``device``, the default, or ``reference``; main.py can pass nothing else) selects the DeviceLoader's sampling
    mode; ``num_workers`` only matters under ``reference``, where it decides which generator stream the reference's draws come from."""
    from torch.utils.data import DataLoader
    mode = sampling_mode()
    rank, world = processing_units()
    units = world if world > 1 else max(1, torch.cuda.device_count())
    total = units * int(batch_size)
    log.info("total batch size is %d (%d processing unit(s) x %d)", total, units, batch_size)
    out = []
    for ds, shuffle in ((train_ds, True), (val_ds, False)):
        if isinstance(ds, DeviceLibSVMDataset):
            out.append(DeviceLoader(ds, total, shuffle=shuffle, rank=rank, world=world, sampling=mode, num_workers=num_workers))
        else:
            out.append(DataLoader(ds, batch_size=total, num_workers=num_workers, shuffle=shuffle))
    return out[0], out[1]
