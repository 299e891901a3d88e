"""Checkpoint files of a training run, and the host-side state that goes into them (``fit(checkpoint_every=..., resume=...)``).

The file is one ``torch.save`` of plain data -- dicts, lists, tuples, strings, numbers, bools, None and tensors -- so that ``load``
can read it with ``weights_only=True``: a checkpoint cannot execute code.  What is not of those types is converted on the way in
(numpy scalars, numpy's and Python's generator states, OrderedDicts) and, where it has to be, back on the way out (``restore_rng``).

The optimizer state is written in a NEUTRAL schema that knows neither the engine nor the flat-buffer layout of the fused step:

    {"kind": "Adam" | "AdamW" | "SGD", "hyper": {lr, betas, eps, weight_decay, momentum, nesterov}, "step": int,
     "state": {parameter name: {"exp_avg", "exp_avg_sq"} | {"momentum_buffer"}}}

with every tensor shaped like its parameter.  ``to_neutral`` / ``from_neutral`` convert a live torch.optim.Adam / AdamW / SGD;
engine.FusedTrainer.state_dict / load_state_dict convert its flat moment buffers.  Any other optimizer is kept as its own
``state_dict()`` under "torch_optimizer" and belongs to the autograd engine.
"""
import collections.abc
import os
import random

import numpy as np
import torch

FORMAT = 1
MAGIC = "allrank_amd.checkpoint"
FILE_NAME = "checkpoint.pt"
ENV_EVERY, ENV_RESUME = "ALLRANK_AMD_CHECKPOINT_EVERY", "ALLRANK_AMD_RESUME"


# ------------------------------------------------------------------------------------------------------------------
# the file
# ------------------------------------------------------------------------------------------------------------------
def plain(value, where="state"):
    """``value`` as the plain data a checkpoint holds: mappings -> dict, numpy scalars -> Python numbers, numpy arrays -> tensors,
    tensors -> detached CPU copies; anything else raises TypeError naming where it sits"""
    if value is None or isinstance(value, (bool, int, float, str)):
        return value
    if isinstance(value, np.generic):
        return value.item()
    if torch.is_tensor(value):
        return value.detach().to("cpu", copy=True).contiguous()
    if isinstance(value, np.ndarray):
        return torch.from_numpy(np.ascontiguousarray(value).copy())
    if isinstance(value, collections.abc.Mapping):
        out = {}
        for k, v in value.items():
            if not isinstance(k, (str, int)) or isinstance(k, bool):
                raise TypeError("checkpoint: key %r of %s is neither a string nor an int" % (k, where))
            out[k] = plain(v, "%s[%r]" % (where, k))
        return out
    if isinstance(value, (list, tuple)):
        items = [plain(v, "%s[%d]" % (where, i)) for i, v in enumerate(value)]
        return tuple(items) if type(value) is tuple else items
    raise TypeError("checkpoint: %s holds a %s, which a checkpoint cannot store" % (where, type(value).__name__))


def save(path, state):
    """write ``state`` (a dict) to ``path`` atomically: the whole file goes to ``path + ".tmp"``, is flushed and fsynced, and then
    replaces ``path`` -- a reader sees the old file or the new one, never a part of either"""
    if not isinstance(state, collections.abc.Mapping):
        raise TypeError("checkpoint.save: the state must be a dict")
    body = plain(state)
    body["magic"], body["format"] = MAGIC, FORMAT
    tmp = path + ".tmp"
    try:
        with open(tmp, "wb") as f:
            torch.save(body, f)
            f.flush()
            os.fsync(f.fileno())
        os.replace(tmp, path)
    finally:
        if os.path.exists(tmp):
            os.remove(tmp)
    return path


def load(path):
    """the dict ``save`` wrote.  A truncated or foreign file, or another format number, raises ValueError naming the path and the
    reason (a missing file raises FileNotFoundError as usual)."""
    if not os.path.exists(path):
        raise FileNotFoundError("checkpoint %s does not exist" % (path,))
    try:
        body = torch.load(path, map_location="cpu", weights_only=True)
    except Exception as exc:                                  # noqa: BLE001 -- whatever the unpickler says about a file that is not one of ours
        raise ValueError("checkpoint %s cannot be read (truncated, or not a checkpoint): %s: %s"
                         % (path, type(exc).__name__, str(exc).splitlines()[0] if str(exc) else "")) from exc
    if not isinstance(body, dict) or body.get("magic") != MAGIC:
        raise ValueError("checkpoint %s is not an allrank_amd checkpoint (no %r marker)" % (path, MAGIC))
    if body.get("format") != FORMAT:
        raise ValueError("checkpoint %s has format %r, this package reads format %d" % (path, body.get("format"), FORMAT))
    return body


# ------------------------------------------------------------------------------------------------------------------
# options
# ------------------------------------------------------------------------------------------------------------------
def options(checkpoint_every=None, resume=None, environ=None):
    """(checkpoint_every: positive int or None, resume: "auto", a path, or None) from fit()'s arguments, with the environment
    standing in for an argument that is None (an unmodified main.py passes only config.training's keys):
    ALLRANK_AMD_CHECKPOINT_EVERY=<positive int>, ALLRANK_AMD_RESUME=auto | <path>.  Anything else raises ValueError."""
    env = os.environ if environ is None else environ
    if checkpoint_every is None:
        raw = env.get(ENV_EVERY)
        if raw:
            try:
                checkpoint_every = int(raw.strip())
            except ValueError:
                raise ValueError("%s must be a positive integer (or unset), got %r" % (ENV_EVERY, raw)) from None
            if checkpoint_every <= 0:
                raise ValueError("%s must be a positive integer (or unset), got %r" % (ENV_EVERY, raw))
    elif isinstance(checkpoint_every, bool) or not isinstance(checkpoint_every, (int, np.integer)) or checkpoint_every <= 0:
        raise ValueError("checkpoint_every must be a positive integer or None, got %r" % (checkpoint_every,))
    if resume is None:
        raw = env.get(ENV_RESUME)
        if raw is not None and raw != "" and not raw.strip():
            raise ValueError("%s must be 'auto' or a path (or unset), got %r" % (ENV_RESUME, raw))
        resume = raw.strip() if raw else None
    elif not isinstance(resume, (str, os.PathLike)) or not str(resume).strip():
        raise ValueError("resume must be 'auto', a path or None, got %r" % (resume,))
    if resume is not None:
        resume = os.fspath(resume)
        if resume.lower() == "auto":
            resume = "auto"
    return (int(checkpoint_every) if checkpoint_every is not None else None), resume


# ------------------------------------------------------------------------------------------------------------------
# generators
# ------------------------------------------------------------------------------------------------------------------
def _is_gpu(device):
    return device is not None and torch.device(device).type == "cuda"


def capture_rng(device=None):
    """the state of every generator a training run draws from outside the fused step: torch's CPU generator (loader shuffles, worker
    base seeds), numpy's global generator (FixLength sampling), Python's ``random``, and the GPU's default generator where ``device``
    is one (the autograd Trainer's nn.Dropout) -- as plain data"""
    kind, key, pos, has_gauss, cached = np.random.get_state()
    ver, internal, gauss = random.getstate()
    return {"torch": torch.get_rng_state().clone(),
            "numpy": {"kind": str(kind), "key": torch.from_numpy(np.asarray(key, dtype=np.uint32).astype(np.int64)), "pos": int(pos),
                      "has_gauss": int(has_gauss), "cached_gaussian": float(cached)},
            "python": {"version": int(ver), "state": torch.tensor([int(v) for v in internal], dtype=torch.int64),
                       "gauss": None if gauss is None else float(gauss)},
            "cuda": torch.cuda.get_rng_state(torch.device(device)).clone() if _is_gpu(device) else None}


def restore_rng(state, device=None):
    """put back what ``capture_rng`` took (the GPU generator only where both the state and ``device`` have one)"""
    torch.set_rng_state(state["torch"].to(torch.uint8).cpu())
    n = state["numpy"]
    np.random.set_state((n["kind"], n["key"].numpy().astype(np.uint32), int(n["pos"]), int(n["has_gauss"]), float(n["cached_gaussian"])))
    p = state["python"]
    random.setstate((int(p["version"]), tuple(int(v) for v in p["state"].tolist()), p["gauss"]))
    if state.get("cuda") is not None and _is_gpu(device):
        torch.cuda.set_rng_state(state["cuda"].to(torch.uint8).cpu(), torch.device(device))


# ------------------------------------------------------------------------------------------------------------------
# the neutral optimizer state
# ------------------------------------------------------------------------------------------------------------------
NEUTRAL_KINDS = ("Adam", "AdamW", "SGD")
_SLOTS = {"Adam": ("exp_avg", "exp_avg_sq"), "AdamW": ("exp_avg", "exp_avg_sq"), "SGD": ("momentum_buffer",)}


def hyper(kind, lr, betas=None, eps=None, weight_decay=0.0, momentum=0.0, nesterov=False):
    """the hyper-parameter block of the schema: what the kind does not use is None / 0 / False whatever the caller holds there"""
    adam = kind in ("Adam", "AdamW")
    return {"lr": float(lr), "betas": [float(b) for b in betas] if adam else None, "eps": float(eps) if adam else None,
            "weight_decay": float(weight_decay), "momentum": 0.0 if adam else float(momentum), "nesterov": False if adam else bool(nesterov)}


def neutral_kind(optimizer):
    """"Adam" / "AdamW" / "SGD" if the schema can hold this optimizer's state (exactly one of those classes, one parameter group,
    no amsgrad / maximize / dampening), else None"""
    if type(optimizer) not in (torch.optim.Adam, torch.optim.AdamW, torch.optim.SGD) or len(optimizer.param_groups) != 1:
        return None
    g = optimizer.param_groups[0]
    if g.get("amsgrad", False) or g.get("maximize", False) or g.get("dampening", 0) != 0:
        return None
    return type(optimizer).__name__


def _named(optimizer, named_parameters):
    """[(name, parameter)] in the order of param_groups[0]["params"]"""
    names = {id(p): n for n, p in named_parameters}
    out = []
    for p in optimizer.param_groups[0]["params"]:
        if id(p) not in names:
            raise ValueError("checkpoint: the optimizer holds a parameter %s that is not one of the model's named parameters"
                             % (tuple(p.shape),))
        out.append((names[id(p)], p))
    return out


def group_hyper(g):
    return {k: plain(v) for k, v in g.items() if k != "params" and (v is None or isinstance(v, (bool, int, float, str, tuple, list)))}


def to_neutral(optimizer, named_parameters):
    """the optimizer's state in the neutral schema (CPU tensors shaped like the parameters; missing per-parameter state -- before the
    first step -- is zeros); a class the schema does not cover: {"kind": class name, "hyper": its group's scalars,
    "torch_optimizer": its own state_dict()}"""
    kind = neutral_kind(optimizer)
    g = optimizer.param_groups[0]
    if kind is None:
        return {"kind": type(optimizer).__name__, "hyper": group_hyper(g) if len(optimizer.param_groups) == 1 else None,
                "torch_optimizer": plain(optimizer.state_dict())}
    steps, state = {}, {}
    for name, p in _named(optimizer, list(named_parameters)):
        st = optimizer.state.get(p, {})
        if "step" in st:
            steps[name] = int(float(st["step"]))
        state[name] = {}
        for slot in _SLOTS[kind]:
            t = st.get(slot)
            state[name][slot] = (torch.zeros(p.shape, dtype=torch.float32) if t is None
                                 else t.detach().to("cpu", torch.float32, copy=True).reshape(p.shape))
    if len(set(steps.values())) > 1 or (steps and len(steps) != len(state)):
        raise ValueError("checkpoint: the optimizer's per-parameter step counts differ (%s) -- the schema holds one step count"
                         % (", ".join("%s: %d" % kv for kv in sorted(steps.items())) or "some parameters have none",))
    return {"kind": kind, "step": next(iter(steps.values())) if steps else 0, "state": state,
            "hyper": hyper(kind, g["lr"], g.get("betas"), g.get("eps"), g.get("weight_decay", 0.0), g.get("momentum", 0.0), g.get("nesterov", False))}


def from_neutral(optimizer, named_parameters, state):
    """load a neutral (or, for the same class, a raw "torch_optimizer") state into a live optimizer.  Hyper-parameters are not
    touched (``check_compatible`` compares them; the learning rate is the caller's to restore)."""
    if "torch_optimizer" in state:
        if type(optimizer).__name__ != state["kind"]:
            raise ValueError("checkpoint: the stored optimizer state is a raw %s state_dict, the live optimizer is a %s"
                             % (state["kind"], type(optimizer).__name__))
        lr = [g["lr"] for g in optimizer.param_groups]
        optimizer.load_state_dict(state["torch_optimizer"])
        for g, v in zip(optimizer.param_groups, lr):
            g["lr"] = v
        return
    kind = neutral_kind(optimizer)
    if kind is None:
        raise ValueError("checkpoint: a neutral %s state cannot be loaded into %s (not a plain Adam / AdamW / SGD with one parameter "
                         "group)" % (state["kind"], type(optimizer).__name__))
    if kind != state["kind"]:
        raise ValueError("checkpoint: optimizer kind: stored %s, live %s" % (state["kind"], kind))
    named = _named(optimizer, list(named_parameters))
    for name, p in named:
        if name not in state["state"] or any(tuple(state["state"][name][s].shape) != tuple(p.shape) for s in _SLOTS[kind]):
            raise ValueError("checkpoint: no optimizer state of shape %s for parameter %s" % (tuple(p.shape), name))
    step = int(state["step"])
    momentum = float(optimizer.param_groups[0].get("momentum", 0.0))
    g = optimizer.param_groups[0]
    on_device = bool(g.get("capturable", False) or g.get("fused", False))      # (where torch keeps the step tensor, optimizer.py)
    for name, p in named:
        src = state["state"][name]
        optimizer.state.pop(p, None)
        if kind == "SGD":
            buf = src["momentum_buffer"]
            if momentum != 0.0 and bool(buf.ne(0).any()):       # (an all-zero buffer is torch's "no buffer yet": same next step)
                optimizer.state[p] = {"momentum_buffer": buf.to(p.device, p.dtype, copy=True)}
        elif step > 0:
            optimizer.state[p] = {"step": torch.tensor(float(step), dtype=torch.float32, device=p.device if on_device else "cpu"),
                                  "exp_avg": src["exp_avg"].to(p.device, p.dtype, copy=True),
                                  "exp_avg_sq": src["exp_avg_sq"].to(p.device, p.dtype, copy=True)}


# ------------------------------------------------------------------------------------------------------------------
# is this file a checkpoint of THIS job?
# ------------------------------------------------------------------------------------------------------------------
def make_meta(named_parameters, optimizer_kind, optimizer_hyper, loss_name, loss_args, clip):
    """the block ``check_compatible`` compares: parameter names and shapes, the optimizer kind and hyper-parameters, the loss and
    its bound keyword arguments, the gradient-clipping norm (None: off)"""
    return {"params": [[str(n), [int(s) for s in p.shape]] for n, p in named_parameters],
            "optimizer": {"kind": str(optimizer_kind), "hyper": plain(dict(optimizer_hyper or {}))},
            "loss": {"name": str(loss_name), "args": plain(dict(loss_args or {}))},
            "clip": float(clip) if clip else None}


def _canon(v):
    if isinstance(v, (list, tuple)):
        return [_canon(x) for x in v]
    if isinstance(v, dict):
        return {k: _canon(x) for k, x in v.items()}
    if isinstance(v, bool) or v is None or isinstance(v, str):
        return v
    if isinstance(v, (int, float)):
        return float(v)
    return v


def check_compatible(saved_meta, live_meta):
    """raise ValueError naming the first difference between the job a checkpoint was written by and the live one: parameter names
    and shapes, optimizer kind and every hyper-parameter except ``lr`` (state, not configuration: the scheduler owns it and it comes
    from the file), loss name and arguments, clipping norm.  A changed config must not silently continue an old run."""
    sp, lp = [(n, tuple(s)) for n, s in saved_meta["params"]], [(n, tuple(s)) for n, s in live_meta["params"]]
    sd, ld = dict(sp), dict(lp)
    for n, s in lp:
        if n not in sd:
            raise ValueError("checkpoint: parameter %s of the live model is not in the checkpoint (it has: %s)"
                             % (n, ", ".join(k for k, _ in sp if k not in ld) or "no other"))
        if sd[n] != s:
            raise ValueError("checkpoint: parameter %s has shape %s in the checkpoint and %s in the live model" % (n, sd[n], s))
    for n, _ in sp:
        if n not in ld:
            raise ValueError("checkpoint: parameter %s of the checkpoint is not in the live model" % (n,))
    so, lo = saved_meta["optimizer"], live_meta["optimizer"]
    if so["kind"] != lo["kind"]:
        raise ValueError("checkpoint: optimizer kind: stored %s, live %s" % (so["kind"], lo["kind"]))
    sh, lh = _canon(so.get("hyper") or {}), _canon(lo.get("hyper") or {})
    for k in sorted(set(sh) | set(lh)):
        if k != "lr" and sh.get(k) != lh.get(k):
            raise ValueError("checkpoint: optimizer hyper-parameter %s: stored %r, live %r" % (k, sh.get(k), lh.get(k)))
    sl, ll = saved_meta["loss"], live_meta["loss"]
    if sl["name"] != ll["name"]:
        raise ValueError("checkpoint: loss: stored %s, live %s" % (sl["name"], ll["name"]))
    sa, la = _canon(sl.get("args") or {}), _canon(ll.get("args") or {})
    for k in sorted(set(sa) | set(la)):
        if sa.get(k, "<unset>") != la.get(k, "<unset>"):
            raise ValueError("checkpoint: loss argument %s: stored %r, live %r" % (k, sa.get(k, "<unset>"), la.get(k, "<unset>")))
    if _canon(saved_meta.get("clip")) != _canon(live_meta.get("clip")):
        raise ValueError("checkpoint: gradient_clipping_norm: stored %r, live %r" % (saved_meta.get("clip"), live_meta.get("clip")))
