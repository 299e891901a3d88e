"""Feature normalisation of resident data sets -- what the reference does in a host script before training
(reproducibility/normalize_features.py: parse three libsvm files, loop over the columns in numpy, dump three new files), done on the
device, in place, on ``DeviceSlates.x_items``.

Per column f, with s = -1 for the columns of ``features_negative`` (normalize_features.py:51-54):
    t = s x,  or  t = log(s x + eps_log)  for a column outside ``features_without_logarithm`` whose s x is >= 0 in EVERY role given (:56-63),
    x <- (t - mean) / (std + eps)  with the mean and the population std of the TRAINING role's t (:65-69),
all in fp64 from the fp32 value, rounded to fp32 once.  Column indices are zero-based, as the script's; indices beyond the data's
feature count are ignored.  The package carries no index lists of its own: ``FeatureNormalizer.from_settings`` reads them from a JSON
file (tests/golden/normalize_web30k.json holds the script's defaults for MSLR-WEB30K).

    nz = FeatureNormalizer.from_settings("normalize_web30k.json")
    nz.fit(train_slates, others=(vali_slates, test_slates))      # the others only feed the sign decision
    for s in (train_slates, vali_slates, test_slates):
        nz.apply(s)                                              # in place; a second apply on the same slates raises
    nz.save("feature_normalization.npz");  FeatureNormalizer.load(...).transform_host(X)      # the same formula in numpy fp64

The three kernel calls (include/ltrx.h, "Feature normalisation"; allrank_amd/csrc/ltrx_featnorm.hip) are stated once, below, in the
form of allrank_amd/kernels.py: one ``ltrx_*`` call on the tensors handed in, the library and the stream as arguments.  They stand here
with the data path, as the loader's calls stand in allrank_amd/data.py.  There is no host fallback: ``fit`` and ``apply`` need device
tensors; ``transform_host`` is for host arrays that never were on the device.
"""
import ctypes
import json
import logging

import numpy as np
import torch

from ._lib import check, ptr as P, workspace

log = logging.getLogger("allrank_amd.normalize")

SETTINGS_KEYS = ("features_without_logarithm", "features_negative", "eps_log", "eps")


# ---- the kernel calls --------------------------------------------------------------------------------------------------
def _host_double(v):
    """a double in host memory and its address (the library reads it before the launch)"""
    d = ctypes.c_double(float(v))
    return d, ctypes.c_void_p(ctypes.addressof(d))


def feature_min_workspace(lib, n, F, like):
    return workspace(lib.ltrx_feature_min_workspace_bytes(n, F), like)


def feature_min(lib, st, x, n, negate, min_out, ws):
    """min_out[f] = min over x[:n, f] of s x; ``x`` is a [rows, F] matrix or a column-slice view with its own row stride"""
    check(lib.ltrx_feature_min(P(x), n, x.shape[1], x.stride(0), P(negate), P(min_out), P(ws), st), "feature_min")


def feature_moments_workspace(lib, n, F, like):
    return workspace(lib.ltrx_feature_moments_workspace_bytes(n, F), like)


def feature_moments(lib, st, x, n, negate, take_log, eps_log, mean_out, std_out, ws):
    """mean_out, std_out (fp64) = the mean and the population std of t over x[:n], two passes"""
    keep, at = _host_double(eps_log)
    check(lib.ltrx_feature_moments(P(x), n, x.shape[1], x.stride(0), P(negate), P(take_log), at, P(mean_out), P(std_out), P(ws), st),
          "feature_moments")
    del keep


def feature_normalize(lib, st, x, n, negate, take_log, eps_log, mean, std, eps):
    """x[:n] = (float)((t - mean) / (std + eps)), in place"""
    keep_a, at_log = _host_double(eps_log)
    keep_b, at_eps = _host_double(eps)
    check(lib.ltrx_feature_normalize(P(x), n, x.shape[1], x.stride(0), P(negate), P(take_log), at_log, P(mean), P(std), at_eps, st),
          "feature_normalize")
    del keep_a, keep_b


# ---- the normaliser ------------------------------------------------------------------------------------------------------
class FeatureNormalizer(object):
    def __init__(self, features_without_logarithm=(), features_negative=(), eps_log=1e-2, eps=1e-6):
        self.features_without_logarithm = tuple(int(i) for i in features_without_logarithm)
        self.features_negative = tuple(int(i) for i in features_negative)
        self.eps_log, self.eps = float(eps_log), float(eps)
        self.negate = self.take_log = self.mean = self.std = None      # numpy, per feature: uint8, uint8, fp64, fp64 -- set by fit
        self.roles, self.no_log_negative = [], []
        self._dev = {}                                                 # device -> (negate, take_log, mean, std) tensors

    # -- settings
    def settings(self):
        return {"features_without_logarithm": list(self.features_without_logarithm), "features_negative": list(self.features_negative),
                "eps_log": self.eps_log, "eps": self.eps}

    @classmethod
    def from_settings(cls, path):
        """a normaliser from a JSON file {"features_without_logarithm": [...], "features_negative": [...], "eps_log": .., "eps": ..}
        (every key optional; any other key is an error)"""
        with open(path) as fh:
            s = json.load(fh)
        unknown = sorted(set(s) - set(SETTINGS_KEYS)) if isinstance(s, dict) else ["<not an object>"]
        if unknown:
            raise ValueError("allrank_amd.normalize: %s: unknown setting(s) %s (known: %s)" % (path, ", ".join(unknown), ", ".join(SETTINGS_KEYS)))
        return cls(**s)

    def flags(self, F):
        """(negate u8[F], log wanted u8[F]) as numpy arrays; listed indices outside [0, F) are ignored"""
        negate, want = np.zeros(F, dtype=np.uint8), np.ones(F, dtype=np.uint8)
        negate[[i for i in self.features_negative if 0 <= i < F]] = 1
        want[[i for i in self.features_without_logarithm if 0 <= i < F]] = 0
        return negate, want

    @property
    def fitted(self):
        return self.mean is not None

    @property
    def n_features(self):
        return None if not self.fitted else int(self.mean.shape[0])

    @property
    def report(self):
        """{"roles": the roles the sign decision saw, "log": how many columns take the logarithm, "no_log_negative": the columns that
        wanted it and hold a negative value}"""
        self._need_fit()
        return {"roles": list(self.roles), "log": int(self.take_log.sum()), "no_log_negative": list(self.no_log_negative)}

    def _need_fit(self):
        if not self.fitted:
            raise RuntimeError("allrank_amd.normalize: the normaliser has no statistics yet -- fit() it or load a saved one")

    # -- device side
    def minimum(self, x):
        """f32[F] on the device: the per-column minimum of s x over the rows of the device matrix ``x`` [n, F] (ltrx_feature_min)"""
        from . import _lib as LB
        LB.require_device(x)
        n, F = int(x.shape[0]), int(x.shape[1])
        negate = torch.from_numpy(self.flags(F)[0]).to(x.device)
        out = torch.empty(F, dtype=torch.float32, device=x.device)
        lib = LB.lib()
        feature_min(lib, LB.stream_of(x), x, n, negate, out, feature_min_workspace(lib, n, F, x))
        return out

    def fit(self, train, others=(), roles=None):
        """statistics from the ``DeviceSlates`` ``train``; ``others`` (DeviceSlates) only take part in the decision whether a column is
        >= 0 everywhere.  ``roles``: names for the record (default train, other1, ...)."""
        mins = [self.minimum(train.x_items)] + [self.minimum(o.x_items) for o in others]
        names = list(roles) if roles is not None else ["train"] + ["other%d" % (k + 1) for k in range(len(others))]
        return self.fit_with_minima(train.x_items, mins, names)

    def fit_with_minima(self, x_train, minima, roles):
        """``fit`` for a caller that reduced the roles itself (``minimum``): ``minima`` = one f32 vector per role, the training role's
        included.  A role with fewer columns than the training role holds zeros there; columns beyond the training role's are ignored."""
        from . import _lib as LB
        LB.require_device(x_train)
        n, F = int(x_train.shape[0]), int(x_train.shape[1])
        negate, want = self.flags(F)
        lo = np.zeros(F, dtype=np.float64)
        for m in minima:
            m = m.detach().cpu().numpy().astype(np.float64)[:F]
            lo[:m.shape[0]] = np.minimum(lo[:m.shape[0]], m)             # (starts at 0: only a negative minimum matters)
        take = (want.astype(bool) & (lo >= 0)).astype(np.uint8)
        lost = [int(i) for i in np.flatnonzero(want.astype(bool) & ~(lo >= 0))]
        for i in lost:
            log.info("Some values of feature no. %d are still < 0 which is why the feature won't be normalized with a logarithm", i)
        dev = x_train.device
        negate_d, take_d = torch.from_numpy(negate).to(dev), torch.from_numpy(take).to(dev)
        mean_d = torch.empty(F, dtype=torch.float64, device=dev)
        std_d = torch.empty(F, dtype=torch.float64, device=dev)
        lib = LB.lib()
        feature_moments(lib, LB.stream_of(x_train), x_train, n, negate_d, take_d, self.eps_log, mean_d, std_d,
                        feature_moments_workspace(lib, n, F, x_train))
        self.negate, self.take_log, self.mean, self.std = negate, take, mean_d.cpu().numpy(), std_d.cpu().numpy()
        self.roles, self.no_log_negative = list(roles), lost
        self._dev = {dev: (negate_d, take_d, mean_d, std_d)}
        return self

    def _device_state(self, dev):
        if dev not in self._dev:
            self._dev[dev] = tuple(torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (self.negate, self.take_log, self.mean, self.std))
        return self._dev[dev]

    def apply(self, slates):
        """normalise ``slates.x_items`` in place (ltrx_feature_normalize).  Slates that a normaliser was applied to carry it as
        ``slates.normalized_by``; applying one again raises."""
        from . import _lib as LB
        self._need_fit()
        if getattr(slates, "normalized_by", None) is not None:
            raise RuntimeError("allrank_amd.normalize: these slates are normalised already; a second pass would standardise twice")
        x = slates.x_items
        LB.require_device(x)
        if int(x.shape[1]) != self.n_features:
            raise ValueError("allrank_amd.normalize: the normaliser was fitted on %d features, the slates hold %d" % (self.n_features, x.shape[1]))
        negate, take, mean, std = self._device_state(x.device)
        feature_normalize(LB.lib(), LB.stream_of(x), x, int(x.shape[0]), negate, take, self.eps_log, mean, std, self.eps)
        slates.normalized_by = self
        return slates

    # -- host side
    def transform_host(self, X):
        """the same formula in numpy: fp64 [n, F] from a host array (values are widened from the dtype they come in)"""
        self._need_fit()
        X = np.asarray(X)
        if X.ndim != 2 or X.shape[1] != self.n_features:
            raise ValueError("allrank_amd.normalize: the normaliser holds %d features, the array is %s" % (self.n_features, X.shape))
        t = X.astype(np.float64)
        t = np.where(self.negate.astype(bool)[None, :], -t, t)
        lg = self.take_log.astype(bool)
        if lg.any():
            t[:, lg] = np.log(t[:, lg] + self.eps_log)
        return (t - self.mean[None, :]) / (self.std[None, :] + self.eps)

    def state_dict(self):
        self._need_fit()
        return dict(self.settings(), negate=self.negate.copy(), take_log=self.take_log.copy(), mean=self.mean.copy(), std=self.std.copy(),
                    roles=list(self.roles), no_log_negative=list(self.no_log_negative))

    def load_state_dict(self, state):
        self.__init__(state["features_without_logarithm"], state["features_negative"], state["eps_log"], state["eps"])
        self.negate, self.take_log = (np.asarray(state[k], dtype=np.uint8).copy() for k in ("negate", "take_log"))
        self.mean, self.std = (np.asarray(state[k], dtype=np.float64).copy() for k in ("mean", "std"))
        if not (self.negate.shape == self.take_log.shape == self.mean.shape == self.std.shape and self.mean.ndim == 1):
            raise ValueError("allrank_amd.normalize: negate, take_log, mean and std must be vectors of one length")
        self.roles = [str(r) for r in state.get("roles", [])]
        self.no_log_negative = [int(i) for i in state.get("no_log_negative", [])]
        return self

    def save(self, path):
        """the state as an .npz (arrays only: loads without pickle)"""
        s = self.state_dict()
        with open(path, "wb") as fh:
            np.savez(fh, features_without_logarithm=np.asarray(s["features_without_logarithm"], dtype=np.int64),
                     features_negative=np.asarray(s["features_negative"], dtype=np.int64), eps_log=np.float64(s["eps_log"]),
                     eps=np.float64(s["eps"]), negate=s["negate"], take_log=s["take_log"], mean=s["mean"], std=s["std"],
                     roles=np.asarray(s["roles"], dtype=np.str_), no_log_negative=np.asarray(s["no_log_negative"], dtype=np.int64))

    @classmethod
    def load(cls, path):
        with np.load(path, allow_pickle=False) as z:
            state = {k: z[k] for k in z.files}
        for k in ("features_without_logarithm", "features_negative", "roles", "no_log_negative"):
            state[k] = state[k].tolist()
        state["eps_log"], state["eps"] = float(state["eps_log"]), float(state["eps"])
        return cls().load_state_dict(state)
