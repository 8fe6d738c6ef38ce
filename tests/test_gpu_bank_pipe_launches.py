"""The launches of the three bank Pipes (sdrhip_pipe_tuner_bank, _am_bank, _nfm_bank), counted: every submission of a uniform run is
ONE tile launch, every ragged submission ONE all-Cross launch where outputs straddle the boundary and ONE tile launch where outputs lie
inside the new block -- and nothing else.  The expected counts come from the seam arithmetic alone (the header comment of fir_submit,
pipes.cpp), restated here; the product is asked only for its debug counters.  The outputs of the same runs are held, bit for bit, to the
models of the Pipes' own tests: the restated firDecimator Pipe on the mixed stream at the pushes' boundaries (oracle/pipes_model.py,
tests/tuner_model.py), then magnitude and the oracle's dcBlocker (AM) or oracle.fm_demod from (0, 0) (narrow-band FM).
Shape: 3 channels, 127 taps (128 prepared), factor 8, AVX order, u8 input, adaptive coalescing off (each push is one submission)."""
import numpy as np
import pytest

import agc_model as AM
import pipe_am_bank_cases as PC
import signals as S
import test_gpu_pipe_am_bank as PA
import test_gpu_pipe_nfm_bank as NF
import test_gpu_pipe_tuner_bank as TB
import tuner_model as TM
from conftest import assert_bit_equal
from oracle import pipes_model as PM

pytestmark = pytest.mark.gpu

LP, D, K, BO = PC.LP, PC.D, 3, 8
SCRIPTS = {"uniform": [2048] * 6, "ragged": [2048, 1000, 3001, 1024, 2047, 4096]}
_cache = {}


def planned_launches(sizes, lp=LP, d=D):
    """(tile, all-Cross) launches of one push per submission.  With E_prev / E the stream positions before / after a block and m_done the
    outputs computed so far: m_end = (E - lp) // d + 1 outputs exist once the block is in, m_split = max(ceil(E_prev / d), m_done) is
    the first output that starts at or after the boundary.  Blocks that all had the first block's size are a uniform run: one launch
    over [m_done, m_end).  Otherwise [m_done, m_split) is the Cross launch and [m_split, m_end) the tile launch, each if non-empty."""
    tile = cross = e_prev = m_done = 0
    uniform = True
    for n in sizes:
        assert n >= lp, "the reference asserts on a block shorter than the filter"
        uniform = uniform and n == sizes[0]
        e = e_prev + n
        m_end = (e - lp) // d + 1 if e >= lp else 0
        m_split = max(-(-e_prev // d), m_done)
        if uniform:
            tile += m_end > m_done
        else:
            cross += m_split > m_done
            tile += m_end > m_split
        e_prev, m_done = e, m_end
    return tile, cross


def counters(hip):
    """(tile, all-Cross) launches of the IQ, envelope and fmDemod forms"""
    return np.array([hip.tuner_bank_launches(), hip.tuner_bank_cross_launches(), hip.am_bank_launches(), hip.am_bank_cross_launches(),
                     hip.nfm_bank_launches(), hip.nfm_bank_cross_launches()])


def models(oracle, table, sizes):
    """{form: every output of the stream pushed as blocks of `sizes`}, computed once per (table, script) and never written"""
    key = (np.asarray(table, np.float32).tobytes(), tuple(sizes))
    if key not in _cache:
        total = sum(sizes)
        m = TM.mix(PC.converted(oracle, "u8", total), table)
        model = PM.FilterModel(oracle, S.taps_decim127(), PM.ORDER_AVX, complex_=True, factor=D)
        out, _ = PM.fir_decimator_pipe(model, PC.cut(m, sizes), BO)
        iq = np.concatenate(out)
        env = AM.magnitude(iq[0::2], iq[1::2])
        forms = {"iq": iq, "env": env, "audio": oracle.dc_blocker(env, 0.0, 0.0)[0], "phase": oracle.fm_demod(iq, last=(0.0, 0.0))}
        for v in forms.values():
            v.setflags(write=False)
        _cache[key] = forms
    return _cache[key]


def make_pipe(hip, kind, tables):
    """-> (the Pipe's raw-call driver, the model's form, its counters' position)"""
    if kind == "tuner_bank":
        return TB.BankPipe(hip, hip.TunerBank(D, S.taps_decim127(), tables), BO, True), "iq", 0
    if kind == "nfm_bank":
        return NF.NfmPipe(hip, NF.nfm_bank(hip, tables), BO, "u8"), "phase", 4
    dc = kind == "am_bank_dc"
    return PA.AmPipe(hip, PA.am_bank(hip, tables, dc=dc), BO, "u8"), "audio" if dc else "env", 2


@pytest.mark.parametrize("script", list(SCRIPTS))
@pytest.mark.parametrize("kind", ["tuner_bank", "am_bank", "am_bank_dc", "nfm_bank"])
def test_launches_follow_the_seam_arithmetic(hip, oracle, kind, script):
    sizes = SCRIPTS[script]
    tile, cross = planned_launches(sizes)
    # (what the arithmetic gives for these scripts, so that a slip in the restatement shows here and not as a product failure)
    assert (tile, cross) == ((6, 0) if script == "uniform" else (6, 5))
    tables = PA.tables_for(K)
    bp, form, at = make_pipe(hip, kind, tables)
    assert bp.rows == K
    bp.p.set_adaptive(0)
    want = np.zeros(6, np.int64)
    want[at], want[at + 1] = tile, cross
    c0 = counters(hip)
    for blk in PC.cut(PC.stream("u8", sum(sizes)), sizes):
        bp.push(blk)
    bp.flush()
    d = (counters(hip) - c0).tolist()
    print(f"{kind}, {script}: launches {d}, planned {want.tolist()}")
    assert d == want.tolist(), f"{kind}, {script}: (IQ tile, IQ cross, env tile, env cross, fm tile, fm cross) launches"
    fpo = 2 if form == "iq" else 1
    nout = ((sum(sizes) - LP) // D + 1) // BO * BO
    for j, t in enumerate(tables):
        got, exp = bp.row(j), models(oracle, t, sizes)[form]
        assert got.size == fpo * nout == exp.size, f"{kind}, {script}: channel {j} yields every whole block"
        assert_bit_equal(got, exp, f"{kind}, {script}: channel {j} against the model")
