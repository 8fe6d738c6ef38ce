"""The numpy model of agc (tests/agc_model.py; Util.hs:325-348 with GHC base's Data.Complex.magnitude at Float) against
float64 hypot, hand-checked magnitudes and a hand-evaluated trajectory -- and the library's exported agc symbols."""
import ctypes as C
import os

import numpy as np

import agc_model
from conftest import assert_bit_equal


def _f32(bits):
    return np.array(bits, dtype=np.uint32).view(np.float32)


def test_magnitude_within_2_ulp_of_hypot():
    """10^6 seeded pairs, half of them with exponents spread over e^+-40 (squares that underflow and overflow in f32)."""
    rng = np.random.default_rng(20240607)
    n = 500_000
    re = np.concatenate([rng.standard_normal(n), rng.standard_normal(n) * np.exp(rng.uniform(-40, 40, n))]).astype(np.float32)
    im = np.concatenate([rng.standard_normal(n), rng.standard_normal(n) * np.exp(rng.uniform(-40, 40, n))]).astype(np.float32)
    got = agc_model.magnitude(re, im).astype(np.float64)
    exact = np.hypot(re.astype(np.float64), im.astype(np.float64))
    exp32 = exact.astype(np.float32)
    # every result is a normal f32 (e^+-40 stays far inside its range), so one ULP is spacing(exp32)
    assert np.all(np.isfinite(exp32) & (exp32 >= np.finfo(np.float32).tiny))
    err = np.abs(got - exact) / np.spacing(exp32).astype(np.float64)
    print(f"worst error {err.max():.3f} ULP over {err.size} pairs")
    assert err.max() <= 2.0, err.max()


def test_magnitude_hand_checked_cases():
    """(re bits, im bits) -> magnitude bits, each worked out by hand from the definition (and with Python floats + struct
    rounding as a second opinion).  The naive sqrtf(re*re + im*im) gives 0 for the fifth and inf for the sixth and seventh."""
    cases = [
        (0x00000000, 0x00000000, 0x00000000),   # a zero sample
        (0x00000000, 0xC0200000, 0x40200000),   # (0, -2.5) -> 2.5
        (0x00000003, 0x3F800000, 0x3F800000),   # (3 * 2^-149, 1) -> 1
        # a denormal beside a zero: exponent 0 = 0 wins the max, nothing is scaled, the square underflows -> 0 (base does that)
        (0x00000003, 0x00000000, 0x00000000),
        (0x0DA24260, 0x0DA24260, 0x0DE57822),   # (1e-30, 1e-30): re*re underflows to 0 in f32; the model gives 1.41421e-30
        (0x7F61B1E6, 0xFE967699, 0x7F6DE740),   # (3e38, -1e38): re*re overflows; the model gives 3.16228e38
        (0x612D78EC, 0x612D78EC, 0x617553B3),   # (2e20, 2e20): both squares overflow; 2.82843e20
        (0x40400000, 0x40800000, 0x40A00000),   # (3, 4) -> 5
    ]
    re, im, exp = (_f32([c[i] for c in cases]) for i in range(3))
    assert_bit_equal(agc_model.magnitude(re, im), exp, "magnitude")
    with np.errstate(over="ignore", under="ignore"):
        naive = np.sqrt(re * re + im * im)
    assert naive[4] == 0.0 and np.isinf(naive[5]) and np.isinf(naive[6])


def test_five_sample_trajectory_by_hand():
    """mu = 0.5, reference = 1, state 1.  The literals come from an evaluation independent of numpy: Python floats with every
    operation rounded to f32 through struct (double rounding is innocuous for +, -, *, sqrt from 53 to 24 bits; ldexp is exact
    in double)."""
    x = _f32([0x3F000000, 0x3E800000, 0xBFC00000, 0x40000000, 0x00000000, 0x00000000, 0x3A83126F, 0xBB449BA6,
              0x3F400000, 0xBDCCCCCD]).view(np.complex64)
    out = _f32([0x3F000000, 0x3E800000, 0xBFEA559A, 0x401C3911, 0x00000000, 0x00000000, 0x3A36286B, 0xBB089E50,
                0x3F65349A, 0xBDF47C60])
    states = _f32([0x3F9C3911, 0x3E478DE0, 0x3F31E378, 0x3F98CDBC, 0x3F9EFEC4])
    got, fin = agc_model.agc(x, 0.5, 1.0, 1.0)
    assert_bit_equal(got.view(np.float32), out, "trajectory outputs")
    assert_bit_equal(fin, states[4], "final state")
    for k in range(1, 5):                                       # every intermediate state, through a prefix run
        _, s = agc_model.agc(x[:k], 0.5, 1.0, 1.0)
        assert_bit_equal(s, states[k - 1], f"state after {k} samples")


def test_ragged_blocks_chain_through_the_state():
    rng = np.random.default_rng(5)
    n = 3000
    x = (0.3 * (rng.standard_normal((3, n)) + 1j * rng.standard_normal((3, n)))).astype(np.complex64)
    state0 = np.array([1.0, 3.0, 0.1], np.float32)
    whole, fin = agc_model.agc(x, 0.05, 0.7, state0)
    cuts = [0, 1, 8, 9, 1000, 1777, n]
    s, parts = state0, []
    for a, b in zip(cuts[:-1], cuts[1:]):
        o, s = agc_model.agc(x[:, a:b], 0.05, 0.7, s)
        parts.append(o)
    assert_bit_equal(np.concatenate(parts, axis=1).view(np.float32), whole.view(np.float32), "blockwise outputs")
    assert_bit_equal(s, fin, "blockwise final state")
    one, f1 = agc_model.agc(x[1], 0.05, 0.7, 3.0)               # a 1-d stream equals its row of the batch
    assert_bit_equal(one.view(np.float32), whole[1].view(np.float32), "1-d stream")
    assert_bit_equal(f1, fin[1], "1-d final state")


def test_library_exports_agc_symbols():
    """No GPU needed: the symbols are looked up in the built library."""
    from sdr_amd import build as B
    if not os.path.exists(B.LIB):
        B.build()
    import sdr_amd.lib as L
    product = C.CDLL(L.LIB_PATH)
    for sym in ("sdrhip_agc_workspace_bytes", "sdrhip_agc_run", "sdrhip_pipe_agc"):
        assert hasattr(product, sym), f"{sym} is not exported by {os.path.basename(L.LIB_PATH)}"
