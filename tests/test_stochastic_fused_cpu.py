"""No GPU: the numpy restatement of the Gumbel generator that tests/test_gpu_stochastic_fused.py pins the device draw to is the
dropout sites' generator (one hash, oracle/dropout_oracle.py), and the seed committed there meets that file's moment bounds."""
import numpy as np

from oracle import dropout_oracle as D
from tests.test_gpu_stochastic_fused import NOISE_SEED, NOISE_SHAPE, gumbel_f64, hash_u32, uniform_f32


def test_restated_hash_is_the_dropout_generator():
    """keep decisions of ``keep_scale`` == (hash >> 8) >= p * 2^24 of the restated hash, for the same seed and step word"""
    n = 50000
    for p, seed, word in ((0.1, 0x1234ABCD, 0), (0.5, NOISE_SEED, 3), (0.03, 0xFFFFFFFF, 0xFFFFFFFE)):
        _, thresh, inv_keep = D.spec(p, seed, word)
        keep = (hash_u32(seed, word, n) >> np.uint64(8)) >= np.uint64(thresh)
        assert np.array_equal(D.keep_scale(p, seed, word, (n,)), np.where(keep, inv_keep, np.float32(0)).astype(np.float32))
        assert abs(float(keep.mean()) - (1 - p)) < 0.01


def test_committed_seed_meets_the_moment_bounds():
    """3(b) of the GPU file on the restated generator: mean within 0.05 of 0.5772, variance within 0.15 of pi^2 / 6; and the largest
    U stays below 1 - 2^-12, where rounding U + 1e-10 in fp32 moves g by less than 5e-7 (the pin of 3(a) evaluates it in fp64)"""
    for word in (0, 1):
        u = uniform_f32(NOISE_SEED, word, int(np.prod(NOISE_SHAPE)))
        g = gumbel_f64(u)
        assert u.dtype == np.float32 and u.size == 16384 and 0.0 <= u.min() and u.max() < 1.0
        assert abs(g.mean() - 0.5772) <= 0.05 and abs(g.var(ddof=1) - np.pi ** 2 / 6) <= 0.15, (word, g.mean(), g.var(ddof=1))
    u = uniform_f32(NOISE_SEED, 0, int(np.prod(NOISE_SHAPE)))
    assert u.max() <= 1 - 2.0 ** -12
    g32 = -np.log(-np.log(u + np.float32(1e-10)) + np.float32(1e-10))             # the device's arithmetic with exact logs
    assert g32.dtype == np.float32
    assert float((np.abs(g32 - gumbel_f64(u)) / np.maximum(1.0, np.abs(gumbel_f64(u)))).max()) <= 5e-7
