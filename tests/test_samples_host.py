"""The sampling generator without a GPU: the numpy twin (tests/samples_ref.py) against the published Philox4x32-10 known answers, its
moments and independence over a block of draws, and the ABI / facade surface of the sampling entries."""
import ctypes

import numpy as np

import samples_ref as sr


def _hex(words):
    return " ".join(f"{int(w):08x}" for w in words)


def test_philox_known_answers():
    """the three Random123 known-answer vectors of philox4x32-10 (kat_vectors: zeros, all ones, the digits of pi)"""
    assert _hex(sr.philox4x32_10((0, 0, 0, 0), (0, 0))) == "6627e8d5 e169c58d bc57ac4c 9b00dbd8"
    ones = 0xFFFFFFFF
    assert _hex(sr.philox4x32_10((ones, ones, ones, ones), (ones, ones))) == "408f276d 41c83b0e a20bc7c6 6d5451fd"
    assert _hex(sr.philox4x32_10((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0))) \
        == "d16cfe09 94fdcceb 5001e420 24126ea1"
    # vectorised counters give what the scalar calls give
    w = sr.philox4x32_10((np.array([0, ones, 0x243F6A88]), np.array([0, ones, 0x85A308D3]), 0, 0), (0, 0))
    assert _hex([w[k][0] for k in range(4)]) == "6627e8d5 e169c58d bc57ac4c 9b00dbd8"
    assert w[0].shape == (3,)


def test_moments_and_independence():
    """rows 0..511 x samples 0..4095 at seed 12345, stream 0 (measured: mean 0.0012, variance 1.0005, fourth moment 2.997, largest
    off-diagonal correlation of the first 64 rows 0.05; one standard error of the mean over 2^21 draws is 0.0007, of the variance 0.001,
    of a correlation over 4096 draws 0.016 with 2016 pairs looked at)"""
    Z = sr.normal_block(12345, 0, 0, 0, 512, 4096)
    assert Z.shape == (512, 4096) and Z.dtype == np.float64 and np.all(np.isfinite(Z))
    print(f"SAMPLES|twin|mean {Z.mean():.4f} var {Z.var():.4f} m4 {np.mean(Z ** 4):.4f}")
    assert abs(Z.mean()) < 0.004
    assert abs(Z.var() - 1.0) < 0.004
    C = np.corrcoef(Z[:64])
    np.fill_diagonal(C, 0.0)
    print(f"SAMPLES|twin|largest correlation {np.abs(C).max():.4f}")
    assert np.abs(C).max() < 0.1
    assert np.abs(Z).max() <= 8.7                      # u1 >= 2^-54: |z| <= sqrt(2 * 54 ln 2)


def test_element_is_a_pure_function_of_its_arguments():
    """a block is its elements: any sub-block, scalar calls; another seed or stream gives other draws; the high words count"""
    Z = sr.normal_block(7, 3, 0, 0, 40, 50)
    assert np.array_equal(sr.normal_block(7, 3, 10, 20, 5, 6), Z[10:15, 20:26])
    assert float(sr.normal(7, 3, 12, 34)) == Z[12, 34]
    for seed, stream in ((8, 3), (7, 4), (7 + 2 ** 32, 3), (7, 3 + 2 ** 32)):
        other = sr.normal_block(seed, stream, 0, 0, 40, 50)
        assert not np.any(other == Z)
        assert abs(np.corrcoef(other.ravel(), Z.ravel())[0, 1]) < 0.1      # 2000 pairs: one standard error is 0.022
    assert sr.normal(7, 3, 1, 2) != sr.normal(7, 3, 2, 1)                   # the row and the sample index are different counter words


def test_uniforms_are_centred_53_bit_cells():
    u1, u2 = sr.uniforms(1, 2, np.arange(1000)[:, None], np.arange(64)[None, :])
    for u in (u1, u2):
        assert np.all(u > 0.0) and np.all(u <= 1.0)
        assert abs(u.mean() - 0.5) < 0.005                                  # 64000 uniforms: one standard error is 0.0011


def test_library_exports_the_sampling_entries():
    import fvgp_amd
    from fvgp_amd import _lib
    _lib.build()
    L = _lib.lib()
    for s in ("fvgp_hip_normal_fill", "fvgp_hip_mvn_sample", "fvgp_hip_mvn_sample_workspace_bytes"):
        assert s in _lib.SYMBOLS and hasattr(L, s)
    assert len(L.fvgp_hip_normal_fill.argtypes) == 9 and L.fvgp_hip_normal_fill.restype is ctypes.c_int
    assert len(L.fvgp_hip_mvn_sample.argtypes) == 15 and L.fvgp_hip_mvn_sample.restype is ctypes.c_int
    assert L.fvgp_hip_mvn_sample_workspace_bytes.restype is ctypes.c_int64
    # the normals, the product and the masked diagonal tiles
    for n, ns in ((1, 1), (128, 128), (129, 1), (300, 300)):
        np_, sp = -(-n // 128) * 128, -(-ns // 128) * 128
        assert _lib.mvn_sample_workspace_bytes(n, ns) == (2 * np_ * sp + 128 * np_) * 8
    assert _lib.mvn_sample_workspace_bytes(0, 1) == -1 and _lib.mvn_sample_workspace_bytes(1, 0) == -1
    # a NULL handle is argument 1 of both calls; nothing is touched
    assert L.fvgp_hip_normal_fill(None, 0, 0, 0, 0, None, 1, 1, 1) == -1
    assert L.fvgp_hip_mvn_sample(None, None, 1, 128, None, 0, 0, 0, 1, None, 1, None, 0, None, 0) == -1
    for m in ("normal_fill", "mvn_sample"):
        assert callable(getattr(_lib.Handle, m))
    for m in ("posterior_samples", "prior_samples"):
        assert callable(getattr(fvgp_amd.GP, m)) and callable(getattr(fvgp_amd.fvGP, m))
