"""CPU-side checks of ltrx_rank_slates_cu: declared in include/ltrx.h, bound from it, exported by the built library, and refusing bad
arguments before any HIP call.  No kernel is launched."""
import ctypes

import pytest

NAME = "ltrx_rank_slates_cu"
FAKE = ctypes.c_void_p(4096)                           # never dereferenced: the argument checks come first


@pytest.fixture(scope="module")
def lib():
    from allrank_amd import _lib, build
    build.build(verbose=False)
    return _lib.lib()


def _call(lib, scores=FAKE, grid=True, resident=False, cu=FAKE, B=2, max_len=8, F=4, L=8, x_out=FAKE, y_out=FAKE, **over):
    a = dict(x=FAKE if grid else None, y=FAKE if grid else None, x_items=FAKE if resident else None, y_items=FAKE if resident else None,
             offsets=FAKE if resident else None, ids=FAKE if resident else None)
    a.update(over)
    return lib.ltrx_rank_slates_cu(scores, a["x"], a["y"], a["x_items"], a["y_items"], a["offsets"], a["ids"], cu, None, B, max_len, F, L,
                                   None, x_out, y_out, None)


def test_the_prototype_is_declared_bound_and_exported(lib):
    from allrank_amd import _lib
    assert NAME in _lib.SIGNATURES and hasattr(ctypes.CDLL(_lib.LIB_PATH), NAME) and hasattr(lib, NAME)
    res, args = _lib.SIGNATURES[NAME]
    assert res is ctypes.c_int and _lib.PROTOTYPES[NAME][1][-1] == "ltrx_stream_t"
    # the ragged layout arguments, in the order every *_cu call has them
    import re
    src = re.sub(r"/\*.*?\*/", "", open(_lib.HEADER_PATH).read(), flags=re.S)
    params = re.search(r"\bint\s+%s\s*\(([^()]*)\)" % NAME, src).group(1)
    names = [re.search(r"(\w+)\s*$", q).group(1) for q in params.split(",")]
    i = names.index("cu_seqlens")
    assert names[i:i + 4] == ["cu_seqlens", "slate_order", "B", "max_len"], names
    assert lib.ltrx_version() == 130


def test_null_pointers_and_bad_sizes_are_invalid(lib):
    assert _call(lib, scores=None) == -1
    assert _call(lib, cu=None) == -1
    assert _call(lib, x_out=None) == -1
    assert _call(lib, y_out=None) == -1
    for B in (0, -3):
        assert _call(lib, B=B) == -1
    for F in (0, -1):
        assert _call(lib, F=F) == -1
    assert _call(lib, max_len=9, L=8) == -1                      # L < max_len
    assert _call(lib, max_len=0, L=8) == -1                      # (no valid call is made here: it would launch)


def test_exactly_one_source_form(lib):
    assert _call(lib, grid=False, resident=False) == -1           # neither
    assert _call(lib, grid=True, resident=True) == -1             # both
    assert _call(lib, grid=True, y=None) == -1                    # half a grid
    assert _call(lib, grid=False, resident=True, ids=None) == -1  # resident without its ids
    assert _call(lib, grid=False, resident=True, offsets=None) == -1
    assert _call(lib, grid=True, ids=FAKE) == -1                  # a grid and a piece of the other form


def test_max_len_above_the_metric_limit_is_unsupported(lib):
    from allrank_amd import _lib
    over = _lib.MAX_METRIC_SLATE_LEN + 1
    assert _call(lib, max_len=over, L=over) == -2
    assert _call(lib, grid=False, resident=True, max_len=over, L=over + 5) == -2
    assert _call(lib, max_len=over, L=over - 1) == -1             # L < max_len is checked first: invalid, whatever the length
