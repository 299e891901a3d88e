"""CPU-side checks of the ragged (cu_seqlens) entry points of the listwise losses and metrics: declared in include/ltrx.h, bound
from it, exported by the built library, and validating their arguments before any HIP call.  No kernel is launched."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["ltrx_listnet_fwd_bwd_cu", "ltrx_approxndcg_fwd_bwd_cu", "ltrx_lambdaloss_fwd_bwd_cu", "ltrx_ndcg_at_cu", "ltrx_mrr_at_cu"]
FAKE = ctypes.c_void_p(4096)                           # never dereferenced: the argument checks come first


@pytest.fixture(scope="module")
def lib():
    from allrank_amd import _lib, build
    build.build(verbose=False)
    return _lib.lib()


def _calls(lib, cu=FAKE, B=1, max_len=8, ptr=FAKE):
    """the five calls with the given layout arguments, every other argument valid; returns their status codes by name"""
    ats = (ctypes.c_int * 2)(1, 5)
    return {
        "ltrx_listnet_fwd_bwd_cu": lib.ltrx_listnet_fwd_bwd_cu(ptr, ptr, cu, None, B, max_len, 1e-10, 1.0, ptr, None, None, ptr, None),
        "ltrx_approxndcg_fwd_bwd_cu": lib.ltrx_approxndcg_fwd_bwd_cu(ptr, ptr, cu, None, B, max_len, 1e-10, 1.0, 1.0, ptr, None, None, ptr, None),
        "ltrx_lambdaloss_fwd_bwd_cu": lib.ltrx_lambdaloss_fwd_bwd_cu(ptr, ptr, cu, None, B, max_len, 1e-10, 3, 0, 1.0, 10.0, 0, 0, None, ptr,
                                                                     None, None, None, ptr, None),
        "ltrx_ndcg_at_cu": lib.ltrx_ndcg_at_cu(ptr, ptr, cu, None, B, max_len, ats, 2, 1.0, ptr, None, None, None, None),
        "ltrx_mrr_at_cu": lib.ltrx_mrr_at_cu(ptr, ptr, cu, None, B, max_len, ats, 2, ptr, ptr, None),
    }


def test_the_five_prototypes_are_declared_bound_and_exported(lib):
    from allrank_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ltrx.h")).read(), flags=re.S)
    h = ctypes.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert re.search(r"\bint\s+%s\s*\(" % name, src), name
        assert name in _lib.SIGNATURES and hasattr(h, name) and hasattr(lib, name), name
        res, args = _lib.SIGNATURES[name]
        assert res is ctypes.c_int and args[-1] is ctypes.c_void_p and _lib.PROTOTYPES[name][1][-1] == "ltrx_stream_t", name
        # y_pred, y_true, cu_seqlens, slate_order, B, max_len lead every ragged call
        assert _lib.PROTOTYPES[name][1][:6] == ["*", "*", "*", "*", "int", "int"], name
    # each mirrors its padded namesake minus pad_value, plus the two layout tables
    for name in NAMES:
        padded = name[:-3]
        assert len(_lib.SIGNATURES[name][1]) == len(_lib.SIGNATURES[padded][1]) - 1 + 2, name
    assert lib.ltrx_version() == 130


def test_null_pointers_and_empty_batches_are_invalid(lib):
    assert set(_calls(lib, cu=None).values()) == {-1}              # no cu_seqlens: not a ragged call
    assert set(_calls(lib, ptr=None).values()) == {-1}             # NULL tensors / outputs / workspace
    assert set(_calls(lib, B=0).values()) == {-1}
    assert set(_calls(lib, B=-3).values()) == {-1}
    assert set(_calls(lib, max_len=0).values()) == {-1}
    ats = (ctypes.c_int * 1)(0)                                    # a cut-off must be positive, as in the padded call
    assert lib.ltrx_ndcg_at_cu(FAKE, FAKE, FAKE, None, 1, 8, ats, 1, 1.0, FAKE, None, None, None, None) == -1
    assert lib.ltrx_ndcg_at_cu(FAKE, FAKE, FAKE, None, 1, 8, None, 1, 1.0, FAKE, None, None, None, None) == -1
    # lambdaLoss: scheme, reduction, log base and eps are checked as in the padded call
    for scheme, red, lg, eps in ((8, 0, 0, 1e-10), (-1, 0, 0, 1e-10), (3, 2, 0, 1e-10), (3, 0, 2, 1e-10), (3, 0, 0, 0.0)):
        assert lib.ltrx_lambdaloss_fwd_bwd_cu(FAKE, FAKE, FAKE, None, 1, 8, eps, scheme, 0, 1.0, 10.0, red, lg, None, FAKE, None, None, None,
                                              FAKE, None) == -1
    assert lib.ltrx_listnet_fwd_bwd_cu(FAKE, FAKE, FAKE, None, 1, 8, 1e-10, 0.0, FAKE, None, None, FAKE, None) == -1     # batch_divisor


def test_max_len_above_the_limits_is_unsupported(lib):
    from allrank_amd import _lib
    over = _calls(lib, max_len=_lib.MAX_LONG_SLATE_LEN + 1)
    assert set(over.values()) == {-2}
    # between the two limits only the metrics object
    assert lib.ltrx_ndcg_at_cu(FAKE, FAKE, FAKE, None, 1, _lib.MAX_METRIC_SLATE_LEN + 1, (ctypes.c_int * 1)(5), 1, 1.0, FAKE, None, None,
                               None, None) == -2
    assert lib.ltrx_mrr_at_cu(FAKE, FAKE, FAKE, None, 1, _lib.MAX_METRIC_SLATE_LEN + 1, (ctypes.c_int * 1)(5), 1, FAKE, FAKE, None) == -2
    assert lib.ltrx_ndcg_at_cu(FAKE, FAKE, FAKE, None, 1, 8, (ctypes.c_int * 17)(*range(1, 18)), 17, 1.0, FAKE, None, None, None, None) == -2


def test_ragged_python_surface_refuses_cpu_tensors_and_bad_layouts(lib):
    import torch
    from allrank_amd import ragged
    x, cu = torch.zeros(5), torch.tensor([0, 2, 5], dtype=torch.int32)
    for fn in (ragged.listNet, ragged.approxNDCGLoss, ragged.lambdaLoss, ragged.ndcg, ragged.dcg, ragged.mrr):
        with pytest.raises(RuntimeError, match="MI355X only"):
            fn(x, x, cu, max_len=3)
    with pytest.raises(ValueError):
        ragged.lambdaLoss(x, x, cu, max_len=3, reduction="median")
    with pytest.raises(KeyError):
        ragged.lambdaLoss(x, x, cu, max_len=3, weighing_scheme="nope")
