"""What the FM bank's 16-bit GPU tests rest on, shown on the CPU (tests/fm_bank_i16_cases.py): the identity table keeps the bits of
a converted sample, the overflow case overflows where it claims to and reaches the audio only through the padded tap, and the
checked ranges hold what they are said to hold."""
import numpy as np
import pytest

import fm_bank_i16_cases as FC
import tuner_model as TM

B = FC.B


def test_identity_table_keeps_the_bits_of_converted_int16(oracle):
    """mix(convert_i16(x), {1, 0}) == convert_i16(x), bit for bit: every int16 value in the I place and in the Q place, against the
    partners -32768, -1, 0, 1, 32767.  (x * 1 - y * 0: the converted values hold no -0, so y * 0 is +0 or -0 and x - (+-0) = x for
    x != 0, and 0 - (+-0) = +0 for the only zero there is, +0; x * 0 + y * 1 likewise.  No subnormal: the smallest is 2^-11.)"""
    vals = np.arange(-32768, 32768, dtype=np.int64).astype(np.int16)
    for partner in (-32768, -1, 0, 1, 32767):
        for place in (0, 1):
            s = np.empty(2 * vals.size, np.int16)
            s[place::2] = vals
            s[1 - place::2] = partner
            c = oracle.convert_i16(s)
            assert not np.signbit(c[c == 0]).any() and (np.abs(c[c != 0]) >= 2.0 ** -11).all()
            m = TM.mix(c, FC.IDENTITY, 12345)
            assert np.array_equal(m.view(np.uint32), c.view(np.uint32)), (partner, place)


def test_the_stream_and_its_forced_sample():
    s = FC.stream()
    assert s.size == 2 * FC.NBLK * B and s.dtype == np.int16
    assert s.min() == -32768 and s.max() == 32767
    blk2 = s[2 * 2 * B + 16:2 * 3 * B - 16]
    assert blk2.min() >= -2048 and blk2.max() <= 2047
    assert -32768 in (int(s[2 * FC.OV_N]), int(s[2 * FC.OV_N + 1])), "the overflow case's sample is a -32768"
    assert FC.OV_N % 8 == 7 and 8 * FC.OV_K + 127 == FC.OV_N


def test_overflow_case(oracle):
    """The table passes the chain's predicate (decided for |x| <= 1) and fails the int16 one; the mixed stream holds an Inf at
    OV_N; the expected audio holds a NaN that is gone when decimator output OV_K -- the one whose window meets OV_N only under the
    padded zero tap -- is replaced by a finite value (what a launch that skipped the tap would compute): the model's tail is
    recomputed from d."""
    t = FC.table("overflow")
    assert np.isfinite(t).all()
    assert FC.chain_says_no_overflow(t) and not FC.i16_says_no_overflow(t)
    for name in FC.NAMES:
        assert FC.chain_says_no_overflow(FC.table(name)) and FC.i16_says_no_overflow(FC.table(name)), name
    s = FC.stream(FC.OV_NBLK)
    blocks = [s[2 * i * B:2 * (i + 1) * B] for i in range(FC.OV_NBLK)]
    mixed, d_blocks = FC.receiver_stages(oracle, blocks, t)
    whole = np.concatenate(mixed).reshape(-1, 2)
    assert np.isinf(whole[FC.OV_N]).any(), "the -32768 sample times 3e37 is an Inf"
    d = np.concatenate(d_blocks).reshape(-1, 2).copy()
    assert np.isnan(d[FC.OV_K]).any(), "0 * Inf under the padded tap"
    audio = FC.tail_from_d(oracle, d_blocks)
    assert audio.size == B
    nan_full = np.isnan(audio)
    d[FC.OV_K] = (0.25, -0.5)
    nb = d.shape[0] // B
    patched = FC.tail_from_d(oracle, [d[i * B:(i + 1) * B].reshape(-1) for i in range(nb)] + ([d[nb * B:].reshape(-1)] if d.shape[0] > nb * B else []))
    assert patched.size == audio.size
    nan_skip = np.isnan(patched)
    gone = nan_full & ~nan_skip
    assert gone.sum() >= 1, "no audio sample tells a skipped padded tap from a walked one: move the case"
    assert not (nan_skip & ~nan_full).any()
    assert np.array_equal(audio[~nan_full].view(np.uint32), patched[~nan_full].view(np.uint32))
    q = int(np.nonzero(gone)[0][0])
    assert FC.OVERFLOW_RANGE[0] <= q < FC.OVERFLOW_RANGE[1], f"the telling output {q} lies outside the range the GPU test runs"
    # the shared model (what the GPU test compares with) is this audio
    assert np.array_equal(FC.model(oracle, "overflow", FC.OV_NBLK).view(np.uint32), audio.view(np.uint32))


@pytest.mark.parametrize("q0,q1,block,stages", FC.CHECKED_RANGES)
def test_checked_ranges_hold_cross_outputs_and_forced_values(q0, q1, block, stages):
    """stages: which FIR stages must have Cross outputs in the range (a run of the first 20 blocks ends before the audio filter's
    first boundary at z sample 8192; the 90-block run and the short seam blocks reach all three)."""
    dec, res, fil = FC.cross_counts(q0, q1, block)
    got = {"d": dec > 0, "r": res > 0, "f": fil > 0}
    for st in stages:
        assert got[st], (q0, q1, block, st)
    if q1 - q0 > 1000:
        assert FC.forced_in(q0, q1, value=-32768) and FC.forced_in(q0, q1, value=32767), (q0, q1)
