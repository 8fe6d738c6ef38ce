"""The CPU restatement (oracle/sdr_oracle.c) against the reference's own compiled C (oracle/_ref, or its recorded answers) on the
value classes that tests/test_oracle_vs_ref.py never feeds: signed zeros, subnormals, tiny and huge normals, overflowing sums,
infinities and NaN in the samples (tests/value_classes.py: salt), zero / subnormal / tiny / huge taps (awkward_taps).  Same structure:
all variants of a family on the same input.  NaN positions must agree, everything else bit for bit (assert_same_classes); each case
also shows on the restatement's output alone that zeros, subnormals, infinities and NaN all occur in it.

convertBladeRFTransmit (convert.c:87-101) gets its restatement here (value_classes.convert_tx_spec): on arguments whose int16 cast is
defined the restatement is the specification and the reference build confirms it; for arguments where the cast is undefined behaviour in
C the reference build's own (recorded) answer is what the library claims to reproduce."""
import numpy as np
import pytest

from oracle.oracle import duplicate
import signals as S
import value_classes as V

N = 8192
TAPS = [("ordinary taps", 0, False), ("level 1", 1, False), ("level 1, last tap 0", 1, True), ("level 2", 2, True)]


def _same(ref_answer, oracle_answer, what):
    V.assert_same_classes(ref_answer, oracle_answer, what)
    V.assert_not_vacuous(oracle_answer, what)


def _inputs(seed, lp):
    rng = np.random.default_rng(seed)
    x, _ = V.salt(rng.uniform(-1, 1, N).astype(np.float32), 1, lp, seed)
    xc, _ = V.salt(rng.uniform(-1, 1, 2 * N).astype(np.float32), 2, lp, seed + 1)
    return rng, x, xc


@pytest.mark.parametrize("ntaps", [32, 128])
@pytest.mark.parametrize("label,level,last_zero", TAPS)
def test_filters(oracle, ref, ntaps, label, level, last_zero):
    rng, x, xc = _inputs(1000 + ntaps + level, ntaps)
    h0 = rng.uniform(-1, 1, ntaps).astype(np.float32)
    h = V.awkward_taps(h0, level, last_zero)
    half = V.awkward_taps(h0[: ntaps // 2], level, last_zero)
    hd = duplicate(h)
    num = N - ntaps + 1
    with ref.canonical():
        for L, sym in ((1, "filterRR"), (4, "filterSSERR"), (8, "filterAVXRR")):
            _same(ref.filt(sym, num, h, x), oracle.filter_rr(L, num, h, x), f"{sym}, {label}")
        for L, sym in ((4, "filterSSESymmetricRR"), (8, "filterAVXSymmetricRR")):
            _same(ref.filt(sym, num, half, x), oracle.filter_sym_rr(L, num, half, x), f"{sym}, {label}")
        _same(ref.filt("filterRC", num, h, xc, True), oracle.filter_rc(1, num, h, xc), f"filterRC, {label}")
        for CL, sym in ((2, "filterSSERC"), (4, "filterAVXRC")):
            _same(ref.filt(sym, num, hd, xc, True), oracle.filter_rc(CL, num, hd, xc), f"{sym}, {label}")
        for CL, sym in ((2, "filterSSERC2"), (4, "filterAVXRC2")):
            _same(ref.filt(sym, num, h, xc, True), oracle.decimate_rc2(CL, num, 1, h, xc), f"{sym}, {label}")
        for CL, sym in ((2, "filterSSESymmetricRC"), (4, "filterAVXSymmetricRC")):
            _same(ref.filt(sym, num, half, xc, True), oracle.decimate_sym_rc(CL, num, 1, half, xc), f"{sym}, {label}")


@pytest.mark.parametrize("factor", [3, 8])
@pytest.mark.parametrize("ntaps", [32, 128])
@pytest.mark.parametrize("label,level,last_zero", TAPS)
def test_decimators(oracle, ref, factor, ntaps, label, level, last_zero):
    rng, x, xc = _inputs(2000 + 31 * factor + ntaps + level, ntaps)
    h0 = rng.uniform(-1, 1, ntaps).astype(np.float32)
    h = V.awkward_taps(h0, level, last_zero)
    half = V.awkward_taps(h0[: ntaps // 2], level, last_zero)
    hd = duplicate(h)
    num = (N - ntaps) // factor + 1
    what = f"/{factor}, {ntaps} taps, {label}"
    with ref.canonical():
        for L, sym in ((1, "decimateRR"), (4, "decimateSSERR"), (8, "decimateAVXRR")):
            _same(ref.decim(sym, num, factor, h, x), oracle.decimate_rr(L, num, factor, h, x), f"{sym} {what}")
        for L, sym in ((4, "decimateSSESymmetricRR"), (8, "decimateAVXSymmetricRR")):
            _same(ref.decim(sym, num, factor, half, x), oracle.decimate_sym_rr(L, num, factor, half, x), f"{sym} {what}")
        _same(ref.decim("decimateRC", num, factor, h, xc, True), oracle.decimate_rc(1, num, factor, h, xc), f"decimateRC {what}")
        for CL, sym in ((2, "decimateSSERC"), (4, "decimateAVXRC")):
            _same(ref.decim(sym, num, factor, hd, xc, True), oracle.decimate_rc(CL, num, factor, hd, xc), f"{sym} {what}")
        for CL, sym in ((2, "decimateSSERC2"), (4, "decimateAVXRC2")):
            _same(ref.decim(sym, num, factor, h, xc, True), oracle.decimate_rc2(CL, num, factor, h, xc), f"{sym} {what}")
        for CL, sym in ((2, "decimateSSESymmetricRC"), (4, "decimateAVXSymmetricRC")):
            _same(ref.decim(sym, num, factor, half, xc, True), oracle.decimate_sym_rc(CL, num, factor, half, xc), f"{sym} {what}")


@pytest.mark.parametrize("I,D,ntaps", [(3, 10, 191), (5, 7, 32)])
@pytest.mark.parametrize("label,level,last_zero", TAPS)
def test_resamplers(oracle, ref, I, D, ntaps, label, level, last_zero):
    lp = -(-ntaps // I // 8) * 8 + 8                   # the longest (padded) polyphase group, in input samples
    rng, x, xc = _inputs(3000 + 101 * I + D + ntaps + level, lp)
    h = V.awkward_taps(rng.uniform(-1, 1, ntaps).astype(np.float32), level, last_zero)
    with ref.canonical():
        for L, sym, CL, csym in ((1, "resample2RR", 1, "resample2RC"), (4, "resampleSSERR", 2, "resampleSSERC"),
                                 (8, "resampleAVXRR", 4, "resampleAVXRC")):
            prep = oracle.prepare_coeffs(L, I, D, h)
            assert prep["padded_len"] <= lp
            ng, period = prep["num_groups"], int(prep["increments"].sum())
            count = ((N - prep["padded_len"] - period) // period) * ng
            start = int(rng.integers(0, ng))
            a, ga = oracle.resample_rr(L, count, prep, start, x)
            b, gb = ref.resample(sym, count, prep, start, x)
            _same(b, a, f"{sym} {I}/{D}, {ntaps} taps, {label}")
            assert ga == gb
            a, ga = oracle.resample_rc(CL, count, prep, start, xc)
            b, gb = ref.resample(csym, count, prep, start, xc, True)
            _same(b, a, f"{csym} {I}/{D}, {ntaps} taps, {label}")
            assert ga == gb


@pytest.mark.parametrize("label,level,last_zero", TAPS)
def test_cross_kernels_are_the_scalar_c_on_the_concatenation(oracle, ref, label, level, last_zero):
    """As test_oracle_vs_ref.test_sequential_order_is_scalar_c: the cross-buffer restatements against the reference's scalar symbols."""
    _, x, xc = _inputs(4000 + level, 128)
    last, nxt = xc[: 2 * 120], xc[2 * 120:]
    h = V.awkward_taps(np.concatenate([S.taps_decim127(), np.zeros(1, np.float32)]), level, last_zero)
    count = (N - 128) // 8 + 1
    with ref.canonical():
        got = oracle.decimate_cross_c(8, h, count, last, nxt)
        _same(ref.decim("decimateRC", count, 8, h, xc, True), got, f"decimateCross == decimateRC, {label}")
        lr, nr = x[:120], x[120:]
        num = N - 128 + 1
        got = oracle.decimate_cross_r(1, h, num, lr, nr)
        _same(ref.filt("filterRR", num, h, x), got, f"filterCross == filterRR, {label}")
        h191 = V.awkward_taps(S.taps_resamp191(), level, last_zero)
        cnt = (N * 3 - 191) // 10 - 2
        got, _ = oracle.resample_cross_r(3, 10, h191, 2, cnt, x[:57], x[57:])
        _same(ref.resample_legacy(cnt, 3, 10, 2, h191, x), got, f"resampleCross == legacy resampleRR, {label}")


def test_scale(oracle, ref):
    _, x, _ = _inputs(5000, 16)
    exps = []
    with ref.canonical():
        for factor in V.SCALE_FACTORS:
            exp = oracle.scale(factor, x)
            exps.append(exp)
            for sym in ("scale", "scaleSSE", "scaleAVX"):
                V.assert_same_classes(ref.scale(sym, factor, x), exp, f"{sym} by {factor!r}")
    # no single factor can show every class (0 * x has no subnormal, 3e38 * x no zero but the zeros'): the five together do
    V.assert_not_vacuous(np.concatenate(exps), "scale, all factors")
    assert np.signbit(oracle.scale(-0.0, np.ones(1, np.float32)))[0], "-0.0 * 1 is -0.0"


def test_convert_tx(ref):
    defined, wild = V.convert_tx_inputs()
    spec = V.convert_tx_spec(defined)
    assert spec.min() == -2048 and spec.max() == 2047 and np.unique(spec).size == 4096
    assert list(V.convert_tx_spec(np.array([-1, 0, -0.0, 1e-40, 1 - 2.0 ** -24, 1], np.float32))) == [-2048, 0, 0, 0, 2047, 2047]
    V.assert_bit_equal(ref.convert_tx(defined), spec, "convertBladeRFTransmit where the cast is defined")
    # undefined behaviour in C: the reference build's answer (recorded where it is not built) is the specification here; the
    # restatement's x86 rule (cvttss2si answers 0x80000000 for NaN and whatever does not fit 32 bits) is shown to describe it
    V.assert_bit_equal(ref.convert_tx(wild), V.convert_tx_spec(wild), "convertBladeRFTransmit on +-1e6, +-3e9, +-Inf, NaN")
