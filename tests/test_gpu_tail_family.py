"""GPU: the kernels specialised for the tail `firResampler 3/10 -> symmetric firFilter (2 x 64 taps) * gain` on every resampler tap
count their predicate admits (fm_tail_shape_ok: 169 .. 192 taps) and on odd block sizes -- the table of tests/tail_family_cases.py.

  * k_audio_tail_rows (AudioTail route 1) and the composition of the row forms (route 2);
  * the chain's three routes: the stage kernels, decimator + k_fm_tail, the one-kernel chain k_fm_chain_small -- the last one also on
    decimators of 125, 126 and 128 taps (three, two and no padding zeros behind the taps);
  * the bank and int16-bank forms of the one-kernel chain (FmBank), against the bank's station-by-station route;
  * 168 and 193 taps, one either side of the family: no fused kernel may launch, and the answer is still the Pipes'.

Every expected value is the restated Pipes' (oracle/pipes_model.py): no device run is a source of expected values.  Every comparison is
bit for bit; every output buffer starts as NaN canaries (gpu_util) and its guard bands are checked.  The launch counters say which kernel
ran.  tests/test_tail_family_cases.py shows on the CPU what the table reaches."""
import numpy as np
import pytest
import torch

import tail_family_cases as TF
from conftest import assert_bit_equal
from gpu_util import CANARY, dev_empty_f32, ptr, to_dev, to_host
from test_gpu_audio_tail import counters as tail_counters, run as run_tail, workspace as tail_workspace
from test_gpu_rows import Rows

pytestmark = pytest.mark.gpu

_dev = {}


def dev(fmt, block):
    """The case's input stream on the device, uploaded once."""
    if (fmt, block) not in _dev:
        _dev[(fmt, block)] = to_dev(TF.bank_stream(fmt, block).copy())       # the table's arrays are read-only
    return _dev[(fmt, block)]


# ---- rows ----------------------------------------------------------------------------------------------------------------------------
def _rows_inputs(key):
    n_y = TF.end_input(TF.Q_MAX - 1, TF.ntaps(key))
    return [TF.y_row(r)[:n_y] for r in range(TF.ROWS)]


@pytest.mark.parametrize("key,block", TF.ROWS_CASES, ids=[f"{k} taps, block {b}" for k, b in TF.ROWS_CASES])
def test_rows_tail_on_every_tap_count(hip, oracle, key, block):
    """Outputs [0, 8400) of 3 rows: route 1 is exactly one launch of k_audio_tail_rows and none of the row forms, route 2 the reverse;
    both are the restated Pipes' composition.  At block 8192 the same range once more as three runs cut at 2047 and 6001, each on a
    buffer that holds exactly its receptive field."""
    tail = hip.AudioTail(TF.I, TF.D, TF.resamp_taps(key), TF.audio_half(), gain=TF.GAIN, block=block)
    assert tail.fused_fits()
    ys = _rows_inputs(key)
    exp = [TF.rows_expected(oracle, key, r, block, TF.GAIN) for r in range(TF.ROWS)]
    for route in (1, 2):
        what = f"{key} taps, block {block}, route {route}"
        outs, (fused, row_forms) = run_tail(hip, tail, ys, 0, TF.Q_MAX, route, exact=False, what=what)
        assert (fused, row_forms) == (1, 0) if route == 1 else (fused == 0 and row_forms >= 2), f"{what}: {fused} fused, {row_forms} row-form launches"
        for r in range(TF.ROWS):
            assert_bit_equal(outs[r], exp[r], f"{what}, row {r} against the restated Pipes")
    if block == 8192:
        what = f"{key} taps, block {block}, route 1 cut at {TF.ROWS_CUTS}"
        outs, (fused, row_forms) = run_tail(hip, tail, ys, 0, TF.Q_MAX, 1, exact=True, cuts=TF.ROWS_CUTS, what=what)
        assert (fused, row_forms) == (len(TF.ROWS_CUTS) + 1, 0), what
        for r in range(TF.ROWS):
            assert_bit_equal(outs[r], exp[r], f"{what}, row {r} against the restated Pipes")
    tail.close()


@pytest.mark.parametrize("key,block", TF.ROWS_LONG_CASES, ids=[f"{k} taps, block {b}" for k, b in TF.ROWS_LONG_CASES])
def test_rows_tail_past_the_second_boundary_of_an_odd_block(hip, oracle, key, block):
    """Outputs [0, 16684): tiles that start past the first buffer boundary, where the kernel's seam positions are real reductions
    modulo the block (below it they are the positions themselves, whatever the block).  Once from 0 on the stream from 0, once from
    8500 on a buffer that holds exactly the receptive field; routes 1 and 2."""
    tail = hip.AudioTail(TF.I, TF.D, TF.resamp_taps(key), TF.audio_half(), gain=TF.GAIN, block=block)
    assert tail.fused_fits()
    ys = [TF.y_row(r, long=True)[:TF.end_input(TF.Q_LONG - 1, TF.ntaps(key))] for r in range(TF.ROWS)]
    exp = [TF.rows_expected(oracle, key, r, block, TF.GAIN, long=True) for r in range(TF.ROWS)]
    for q0, exact in ((0, False), (TF.Q_LONG_START, True)):
        for route in (1, 2):
            what = f"{key} taps, block {block}, outputs [{q0},{TF.Q_LONG}), route {route}"
            outs, (fused, row_forms) = run_tail(hip, tail, ys, q0, TF.Q_LONG, route, exact=exact, what=what)
            assert (fused, row_forms) == (1, 0) if route == 1 else (fused == 0 and row_forms >= 2), f"{what}: {fused} fused, {row_forms} row-form launches"
            for r in range(TF.ROWS):
                assert_bit_equal(outs[r], exp[r][q0:], f"{what}, row {r} against the restated Pipes")
    tail.close()


# ---- chains --------------------------------------------------------------------------------------------------------------------------
CHAIN_ROUTES = ("stage", "tail", "small")
CHAIN_COUNTERS = ("sdrhip_debug_small_chain_launches", "sdrhip_debug_fused_tail_launches", "sdrhip_debug_audio_tail_launches",
                  "sdrhip_debug_resample_cycle_launches", "sdrhip_debug_fused_demod_launches")
# what one run adds to CHAIN_COUNTERS.  The stage route of these runs is the 3/10 tile kernel of kernels_chain.hip with a stand-alone
# fmDemod in front: the thread-per-cycle kernel serves no 3/10, and fmDemod moves into the loader from 2^18 resampler outputs on
EXPECTED_LAUNCHES = {"stage": (0, 0, 0, 0, 0), "tail": (0, 1, 0, 0, 0), "small": (1, 0, 0, 0, 0)}


def chain_counters(hip):
    return tuple(int(getattr(hip.lib, n)()) for n in CHAIN_COUNTERS)


def set_route(ch, route):
    """stage: the stage kernels; tail: decimator + k_fm_tail; small: the one-kernel chain; auto: the library's own choice."""
    ch.set_small_chain({"small": 1, "auto": 2}.get(route, 0))
    ch.set_fused_tail({"tail": 1, "auto": 2, "small": 1}.get(route, 0))


def run_chain(hip, ch, d_in, n_in, q0, q1):
    """-> (audio [q0, q1), what the run added to CHAIN_COUNTERS)"""
    ws_bytes = ch.workspace_bytes(n_in)
    ws = torch.empty(max(ws_bytes, 16), dtype=torch.uint8, device="cuda")
    out = dev_empty_f32(q1 - q0)
    c0 = chain_counters(hip)
    ch.run(ptr(d_in), 0, n_in, ptr(out), q0, q1, ptr(ws), ws_bytes)
    got = to_host(out)
    return got, tuple(b - a for a, b in zip(c0, chain_counters(hip)))


def _chain(hip, key, block, decim=127):
    return hip.FmChain(TF.DECIM, TF.decim_taps(decim), TF.I, TF.D, TF.resamp_taps(key), TF.audio_half(), TF.GAIN, block)


def _sub_ranges(key, block, q1):
    rng = np.random.default_rng(7700 + 16 * TF.ntaps(key) + block % 16)
    out = []
    for _ in range(6):
        a = int(rng.integers(0, q1 - 10))
        out.append((a, int(min(q1, a + rng.integers(1, 9000)))))
    return out


@pytest.mark.parametrize("key,block", TF.CHAIN_CASES, ids=[f"{k} taps, block {b}" for k, b in TF.CHAIN_CASES])
def test_chain_routes_on_tap_counts_and_odd_blocks(hip, oracle, key, block):
    """70 source blocks of FM signal.  Each route is held to PM.fm_receiver over the audio the Pipes yield, the routes to each other
    over every output of the plan and over six seeded sub-ranges that start and end inside tiles."""
    total = TF.CHAIN_NBLK * block
    d = dev("u8", block)
    exp = TF.chain_expected(oracle, key, block)
    ch = _chain(hip, key, block)
    q0, q1, halo = ch.plan(0, total, total)
    assert (q0, halo) == (0, 0) and q1 >= exp.size == block
    for a, b in [(0, q1)] + _sub_ranges(key, block, q1):
        got = {}
        for route in CHAIN_ROUTES:
            set_route(ch, route)
            got[route], launches = run_chain(hip, ch, d, total, a, b)
            what = f"{key} taps, block {block}, outputs [{a},{b}), route {route}"
            assert launches == EXPECTED_LAUNCHES[route], f"{what}: launches {dict(zip(CHAIN_COUNTERS, launches))}"
            if (a, b) == (0, q1):
                assert_bit_equal(got[route][:exp.size], exp, f"{what} against the restated Pipes")
            elif a < exp.size:
                hi = min(b, exp.size)
                assert_bit_equal(got[route][:hi - a], exp[a:hi], f"{what} against the restated Pipes")
        for route in CHAIN_ROUTES[1:]:
            assert_bit_equal(got[route], got["stage"], f"{key} taps, block {block}, outputs [{a},{b}): route {route} against the stage kernels")
    ch.close()


@pytest.mark.parametrize("key,block", TF.CHAIN_LONG_CASES, ids=[f"{k} taps, block {b}" for k, b in TF.CHAIN_LONG_CASES])
def test_chain_routes_past_the_second_boundary_of_an_odd_block(hip, oracle, key, block):
    """100 source blocks: two audio blocks of the restated Pipes, the second behind the filter's second buffer boundary, where a
    tile's seam position is a real reduction modulo the block.  Each route against the Pipes."""
    total = TF.CHAIN_LONG_NBLK * block
    d = to_dev(TF.chain_u8(block, TF.CHAIN_LONG_NBLK).copy())
    exp = TF.chain_expected(oracle, key, block, nblk=TF.CHAIN_LONG_NBLK)
    ch = _chain(hip, key, block)
    q0, q1, _ = ch.plan(0, total, total)
    assert q0 == 0 and q1 >= exp.size == 2 * block
    for route in CHAIN_ROUTES:
        set_route(ch, route)
        for a in (0, block + 1):
            got, launches = run_chain(hip, ch, d, total, a, exp.size)
            what = f"{key} taps, block {block}, outputs [{a},{exp.size}), route {route}"
            assert launches == EXPECTED_LAUNCHES[route], f"{what}: launches {dict(zip(CHAIN_COUNTERS, launches))}"
            assert_bit_equal(got, exp[a:], f"{what} against the restated Pipes")
    ch.close()


@pytest.mark.parametrize("decim", TF.DECIM_COUNTS)
def test_one_kernel_chain_on_other_decimator_tap_counts(hip, oracle, decim):
    """125, 126 and 128 decimator taps (all 128 prepared): the one-kernel chain's skip of the last, zero tap meets three, two and no
    padding zeros.  170 resampler taps, block 7315."""
    key, block = TF.DECIM_CASE
    total = TF.CHAIN_NBLK * block
    d = dev("u8", block)
    exp = TF.chain_expected(oracle, key, block, decim)
    ch = _chain(hip, key, block, decim)
    q0, q1, _ = ch.plan(0, total, total)
    assert q0 == 0 and q1 >= exp.size == block
    got = {}
    for route in ("stage", "small"):
        set_route(ch, route)
        got[route], launches = run_chain(hip, ch, d, total, 0, q1)
        what = f"{decim} decimator taps, route {route}"
        assert launches == EXPECTED_LAUNCHES[route], f"{what}: launches {dict(zip(CHAIN_COUNTERS, launches))}"
        assert_bit_equal(got[route][:exp.size], exp, f"{what} against the restated Pipes")
    assert_bit_equal(got["small"], got["stage"], f"{decim} decimator taps: the one-kernel chain against the stage kernels")
    ch.close()


# ---- banks ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt,key,block", TF.BANK_CASES, ids=[f"{f}, {k} taps, block {b}" for f, k, b in TF.BANK_CASES])
def test_bank_forms_on_tap_counts_and_an_odd_block(hip, oracle, fmt, key, block):
    """Two stations.  The banked launch (one launch of the bank form of k_fm_chain_small; on int16 input the int16 form) against the
    bank's station-by-station route and against the restated Pipes with the oscillator stage."""
    total = TF.CHAIN_NBLK * block
    d = dev(fmt, block)
    bank = hip.FmBank(TF.DECIM, TF.decim_taps(), TF.I, TF.D, TF.resamp_taps(key), TF.audio_half(), [TF.table(n) for n in TF.STATIONS], TF.GAIN, block)
    K = bank.stations()
    q0, q1, halo = bank.plan(0, total, total)
    assert (K, q0, halo) == (len(TF.STATIONS), 0, 0) and q1 >= block
    stride = q1 + 5
    ws_bytes = bank.workspace_bytes(total)
    ws = torch.empty(max(ws_bytes, 16), dtype=torch.uint8, device="cuda")
    rows = {}
    for route in (1, 2):
        bank.set_route(route)
        out = dev_empty_f32(K * stride)
        c0 = (hip.fm_bank_launches(), hip.fm_bank_i16_launches(), int(hip.lib.sdrhip_debug_fused_tail_launches()))
        (bank.run if fmt == "u8" else bank.run_i16)(ptr(d), 0, total, ptr(out), stride, 0, q1, ptr(ws), ws_bytes)
        whole = to_host(out).reshape(K, stride)
        c1 = (hip.fm_bank_launches(), hip.fm_bank_i16_launches(), int(hip.lib.sdrhip_debug_fused_tail_launches()))
        delta = tuple(b - a for a, b in zip(c0, c1))
        what = f"{fmt}, {key} taps, block {block}, route {route}"
        assert delta == ((1, int(fmt == "i16"), 0) if route == 1 else (0, 0, delta[2])), f"{what}: launches {delta}"
        assert (whole[:, q1:].view(np.uint32) == CANARY).all(), f"{what}: a float between the rows was written"
        rows[route] = whole[:, :q1]
        for j, name in enumerate(TF.STATIONS):
            exp = TF.bank_expected(oracle, fmt, name, key, block)
            assert exp.size == block
            assert_bit_equal(rows[route][j][:exp.size], exp, f"{what}, station {j} ({name}) against the restated Pipes")
    for j in range(K):
        assert_bit_equal(rows[1][j], rows[2][j], f"{fmt}, {key} taps, block {block}, station {j}: banked launch against station by station")
    bank.close()


# ---- the predicate's edges -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", TF.EDGES)
def test_a_count_outside_the_family_reaches_no_fused_kernel(hip, oracle, n):
    """168 taps prepare to 56-float groups, 193 to 72-float groups: fm_tail_shape_ok says no.  AudioTail route 1 is refused and writes
    nothing; routes 2 and 0 launch no fused kernel.  A chain on its automatic routes and with both fused kernels forced launches none
    of them, on a whole run and on a short one that the automatic rules would hand to them.  Every result is the restated Pipes'."""
    block = TF.EDGE_BLOCK
    tail = hip.AudioTail(TF.I, TF.D, TF.resamp_taps(n), TF.audio_half(), gain=TF.GAIN, block=block)
    assert not tail.fused_fits()
    ys = _rows_inputs(n)
    exp = [TF.rows_expected(oracle, n, r, block, TF.GAIN) for r in range(TF.ROWS)]
    src, dst = Rows(TF.ROWS, ys[0].size, 0, 0, host=ys), Rows(TF.ROWS, TF.Q_MAX, 0, 0)
    tail.set_route(1)
    c0 = tail_counters(hip)
    with pytest.raises(hip.SdrHipError, match="route 1"):
        tail.run_rows(src.view, dst.view, 0, TF.Q_MAX, workspace=tail_workspace(tail, TF.ROWS, ys[0].size))
    assert tail_counters(hip) == c0 and dst.untouched(), f"{n} taps: a refused call launched or wrote"
    for route in (2, 0):
        what = f"{n} taps, rows, route {route}"
        outs, (fused, row_forms) = run_tail(hip, tail, ys, 0, TF.Q_MAX, route, exact=False, what=what)
        assert fused == 0 and row_forms >= 2, what
        for r in range(TF.ROWS):
            assert_bit_equal(outs[r], exp[r], f"{what}, row {r} against the restated Pipes")
    tail.close()

    total = TF.CHAIN_NBLK * block
    d = dev("u8", block)
    exp = TF.chain_expected(oracle, n, block)
    ch = _chain(hip, n, block)
    q0, q1, _ = ch.plan(0, total, total)
    assert q0 == 0 and q1 >= exp.size == block
    for route in ("auto", "small", "tail"):
        set_route(ch, route)
        for a, b in ((0, q1), (0, 600), (2047, 2047 + 153)):
            got, launches = run_chain(hip, ch, d, total, a, b)
            what = f"{n} taps, chain on route {route}, outputs [{a},{b})"
            assert launches == (0, 0, 0, 0, 0), f"{what}: launches {dict(zip(CHAIN_COUNTERS, launches))}"
            hi = min(b, exp.size)
            assert_bit_equal(got[:hi - a], exp[a:hi], f"{what} against the restated Pipes")
    ch.close()
