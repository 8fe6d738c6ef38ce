"""GPU parity of the receiver bank on 16-bit signed IQ (sdrhip_fm_bank_run_i16).  The definition is the specification: station j's
row is, bit for bit, on every route and for any tile size, the composition sdrhip_tuner_run_i16 -> sdrhip_fm_demod_run ->
sdrhip_resampler_run -> sdrhip_filter_run -> sdrhip_scale_run driven by hand with table j over the same (s0, n_in, q0, q1).  Every
comparison here is against that composition run on the same device, or against the restated Pipes on oracle.convert_i16 of the stream
(tests/fm_bank_i16_cases.py) -- never against the bank itself.  Chain arguments and tables are those of
tests/test_gpu_tuned_chain.py; the stream is tuner_i16_cases.stream_i16; every output sits between canaries (gpu_util)."""
import numpy as np
import pytest
import torch

import fm_bank_i16_cases as FC
import signals as S
import test_gpu_tuned_chain as T
import tuner_i16_cases as IC
from conftest import assert_bit_equal
from gpu_util import CANARY, dev_empty_f32, ptr, to_dev, to_host

pytestmark = pytest.mark.gpu

B = FC.B
_dev = {}
_refs = {}


def dev(key="stream"):
    """Device copies, uploaded once: the 96-block stream; `plus1`: one int16 pair in front of it (the stream then starts 4 bytes
    past a 16-byte boundary); `long`: a 140-block stream of its own for the 39322-output edge."""
    if key not in _dev:
        if key == "stream":
            _dev[key] = to_dev(FC.stream())
        elif key == "plus1":
            _dev[key] = to_dev(np.concatenate([np.zeros(2, np.int16), FC.stream()]))
        elif key == "long":
            _dev[key] = to_dev(IC.stream_i16(140 * B))
    return _dev[key]


def _bank(hip, names, block=B):
    return hip.FmBank(8, S.taps_decim127(), 3, 10, S.taps_resamp191(), S.taps_audio_half64(), [FC.table(n) for n in names], FC.GAIN, block)


def compose(hip, name, p_in, s0, q0, q1, block=B, key="stream"):
    """The definition, by hand (computed once per run and table, never written).  p_in: device address of stream sample s0."""
    k = (name, block, s0, q0, q1, key)
    if k not in _refs:
        order = hip.ORDER_AVX
        t = hip.Tuner(8, S.taps_decim127(), FC.table(name), order)
        res = hip.Resampler(3, 10, S.taps_resamp191(), order)
        filt = hip.Filter(S.taps_audio_half64(), order, sym=True)
        r = FC.ranges(q0, q1)
        m1, ky0, ky1, kd0, kd1 = r["m1"], r["ky0"], r["ky1"], r["kd0"], r["kd1"]
        assert m1 == q1 + filt.num_coeffs - 1 and ky0 == res.in_offset(q0) and ky1 == res.in_offset(m1 - 1) + FC.NLOOP
        d = dev_empty_f32(2 * (kd1 - kd0))
        t.run_i16(p_in, s0, ptr(d), kd0, kd1, block)
        y = dev_empty_f32(ky1 - ky0)
        hip.check(hip.lib.sdrhip_fm_demod_run(None, ptr(d), kd0, ptr(y), ky0, ky1, 0.0, 0.0), "sdrhip_fm_demod_run")
        z = dev_empty_f32(m1 - q0)
        res.run(ptr(y), ky0, ptr(z), q0, m1, block, out_block=block)
        a = dev_empty_f32(q1 - q0)
        filt.run(ptr(z), q0, ptr(a), q0, q1, block)
        out = dev_empty_f32(q1 - q0)
        hip.check(hip.lib.sdrhip_scale_run(None, FC.GAIN, ptr(a), ptr(out), q1 - q0), "sdrhip_scale_run")
        o = to_host(out)
        o.setflags(write=False)
        _refs[k] = o
    return _refs[k]


def run_bank(hip, bank, p_in, s0, n_in, q0, q1, stride=None, workspace=True, ws_bytes=None):
    """-> (rows [stations, q1 - q0], the whole output buffer as uint32)"""
    K, n = bank.stations(), q1 - q0
    stride = n if stride is None else stride
    out = dev_empty_f32(K * stride)
    wsb = (bank.workspace_bytes(n_in) if ws_bytes is None else ws_bytes) if workspace else 0
    ws = torch.empty(max(wsb, 16), dtype=torch.uint8, device="cuda") if workspace else None
    bank.run_i16(p_in, s0, n_in, ptr(out), stride, q0, q1, ptr(ws) if workspace else None, wsb)
    whole = to_host(out)                                       # checks the guard bands around the buffer
    return whole.reshape(K, stride)[:, :n], whole.view(np.uint32)


def same_bits(got, exp, what):
    """bit for bit; a NaN is compared by position"""
    got, exp = np.asarray(got), np.asarray(exp)
    assert got.shape == exp.shape, what
    gn, en = np.isnan(got), np.isnan(exp)
    assert np.array_equal(gn, en), f"{what}: NaNs at {np.nonzero(gn)[0][:8]} against {np.nonzero(en)[0][:8]}"
    bad = got.view(np.uint32)[~gn] != exp.view(np.uint32)[~gn]
    assert not bad.any(), f"{what}: {int(bad.sum())} of {got.size} floats differ, first at {int(np.nonzero(bad)[0][0])}"


def check_rows(hip, names, rows, p_in, s0, q0, q1, what, **kw):
    assert rows.shape == (len(names), q1 - q0)
    for j, name in enumerate(names):
        same_bits(rows[j], compose(hip, name, p_in, s0, q0, q1, **kw), f"{what}: station {j} ({name}) vs the hand-driven composition")


def counters(hip):
    return (hip.fm_bank_launches(), hip.fm_bank_i16_launches(), int(hip.lib.sdrhip_debug_small_chain_launches()), hip.tuner_i16_launches(),
            hip.tuner_fused_launches())


# ---- 1 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 3, 32])
def test_banked_route_equals_the_definition(hip, K):
    """20 blocks from the stream's start.  Per run exactly one banked launch and one int16 launch, none of a chain's one-kernel
    route and none of the tuner's.  Run twice."""
    names = {1: ["shift 1/65536"], 3: ["shift -3/1000", "shift 5/8313", "shift -3/1000"], 32: [FC.NAMES[j % len(FC.NAMES)] for j in range(32)]}[K]
    total = 20 * B
    d = dev()
    bank = _bank(hip, names)
    q0, q1, halo = bank.plan(0, total, total)
    assert (q0, q1, halo) == (0, 5994, 0)
    for name in set(names):
        compose(hip, name, ptr(d), 0, q0, q1)                   # the references first: they launch the tuner's kernels
    bank.set_route(1)
    for rep in range(2):
        c0 = counters(hip)
        rows, _ = run_bank(hip, bank, ptr(d), 0, total, q0, q1, workspace=False)
        c1 = counters(hip)
        assert c1[0] == c0[0] + 1 and c1[1] == c0[1] + 1, "one banked launch, and it is an int16 one"
        assert c1[2:] == c0[2:], "a banked run launched a chain's or a tuner's kernel"
        check_rows(hip, names, rows, ptr(d), 0, q0, q1, f"{K} stations, run {rep}")
    if K == 3:
        assert not np.array_equal(rows[0], rows[1])


# ---- 2 ---------------------------------------------------------------------------------------------------------------------------
def test_against_the_restated_pipes(hip, oracle):
    """2 stations on 90 blocks (2 audio blocks each) against the restated Pipes with the oscillator stage on convert_i16 of the
    stream; one station of {1, 0} against the restated Pipes WITHOUT the oscillator stage."""
    total = 90 * B
    d = dev()
    for names, with_osc in ((["shift 1/4", "shift -3/1000"], True), (["identity"], False)):
        bank = _bank(hip, names)
        q0, q1, _ = bank.plan(0, total, total)
        assert q0 == 0 and q1 >= 2 * B
        bank.set_route(1)
        b0 = hip.fm_bank_i16_launches()
        rows, _ = run_bank(hip, bank, ptr(d), 0, total, 0, q1)
        assert hip.fm_bank_i16_launches() == b0 + 1
        for j, name in enumerate(names):
            exp = FC.model(oracle, name, with_osc=with_osc)
            assert exp.size == 2 * B
            same_bits(rows[j][:exp.size], exp, f"station {j} ({name}) vs the restated Pipes, oscillator stage: {with_osc}")


# ---- 3 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("q0,q1", [(1000, 3001), (0, 2000), (500, 501), (158, 4251)])
def test_edges_of_a_launch(hip, q0, q1):
    names = ["shift -3/1000", "random, period 5", "shift 5/8313"]
    total = 20 * B
    d = dev()
    bank = _bank(hip, names)
    for tile in (0, 3, 96, 159):
        bank.set_route(1, 0, tile)
        b0 = hip.fm_bank_i16_launches()
        rows, _ = run_bank(hip, bank, ptr(d), 0, total, q0, q1)
        assert hip.fm_bank_i16_launches() == b0 + 1
        check_rows(hip, names, rows, ptr(d), 0, q0, q1, f"outputs [{q0},{q1}), tile of {tile}")


# ---- 4 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("start", ["stream start", "s0 = 4 * 10001", "two samples more"])
def test_both_ragged_ends(hip, start):
    """The buffer holds exactly the receptive field of [q0, q1) (from s0 on); the stream with its top bits flipped lies before and
    behind it.  At the stream's start the first tile begins before sample 0; at s0 = 4 * 10001 (a multiple of 4, not of 8) the
    first tile begins 12 samples before the buffer.  `two samples more`: the buffer ends inside a 16-byte vector.  The audio is
    that of the whole stream."""
    names = ["shift -3/1000", "shift 1/65536"]
    s = FC.stream(20)
    if start == "stream start":
        q0, q1, s0, extra = 0, 700, 0, 0
    elif start == "s0 = 4 * 10001":
        q0, q1, s0, extra = 1501, 2300, 4 * 10001, 0
    else:
        q0, q1, s0, extra = 1500, 2111, FC.ranges(1500, 2111)["n_lo"], 2
    r = FC.ranges(q0, q1)
    assert s0 <= r["n_lo"] < s0 + 24 and s0 % 4 == 0
    n_in = r["n_hi"] - s0 + extra
    pad = 64                                                    # samples of flipped stream in front, also at the stream's start
    flipped = (s.view(np.uint16) ^ 0x8000).view(np.int16)
    host = np.concatenate([flipped[:2 * pad], flipped]).copy()
    host[2 * (pad + s0):2 * (pad + s0 + n_in)] = s[2 * s0:2 * (s0 + n_in)]
    dd = to_dev(host)
    p_in = ptr(dd) + 4 * (pad + s0)
    assert p_in % 16 == 0
    bank = _bank(hip, names)
    whole = dev()
    for tile in (0, 96):
        bank.set_route(1, 0, tile)
        b0 = hip.fm_bank_i16_launches()
        rows, _ = run_bank(hip, bank, p_in, s0, n_in, q0, q1, workspace=False)
        assert hip.fm_bank_i16_launches() == b0 + 1
        check_rows(hip, names, rows, ptr(whole), 0, q0, q1, f"{start}, tile {tile}: exactly the receptive field vs the whole stream")
    # one sample less at the far end is refused with nothing written
    out = dev_empty_f32(2 * (q1 - q0))
    rc = hip.lib.sdrhip_fm_bank_run_i16(bank.h, None, p_in, s0, r["n_hi"] - s0 - 1, ptr(out), q1 - q0, q0, q1, None, 0)
    assert rc == -1 and (to_host(out).view(np.uint32) == CANARY).all()


# ---- 5 ---------------------------------------------------------------------------------------------------------------------------
def test_far_stream_position(hip):
    s0 = 2 ** 33 + 4 * 12345
    assert s0 % 4 == 0 and s0 % 8 != 0 and s0 % 1000 != s0 % 65536
    n_in = 6 * B
    names = ["shift -3/1000", "shift 1/65536"]
    d = dev()
    bank = _bank(hip, names)
    end = s0 + n_in
    Q0, Q1, halo = bank.plan(s0, end, end)
    assert halo == 0 and Q1 - Q0 > 1500 and Q0 > 2 ** 28
    bank.set_route(1)
    b0 = hip.fm_bank_i16_launches()
    full, _ = run_bank(hip, bank, ptr(d), s0, n_in, Q0, Q1)
    assert hip.fm_bank_i16_launches() == b0 + 1
    check_rows(hip, names, full, ptr(d), s0, Q0, Q1, "far position")
    near, _ = run_bank(hip, bank, ptr(d), 0, n_in, *bank.plan(0, n_in, n_in)[:2])
    for j in range(2):
        assert not np.array_equal(near[j][:1000], full[j][:1000]), "the position did not reach the oscillator"


# ---- 6 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("block", [0, 192, 200, B])
def test_seams(hip, block):
    names = ["shift -3/1000", "shift 1/4", "random, period 5"]
    total = 20 * B
    d = dev()
    bank = _bank(hip, names, block)
    q0, q1, _ = bank.plan(0, total, total)
    bank.set_route(1)
    b0 = hip.fm_bank_i16_launches()
    rows, _ = run_bank(hip, bank, ptr(d), 0, total, q0, q1)
    assert hip.fm_bank_i16_launches() == b0 + 1
    check_rows(hip, names, rows, ptr(d), 0, q0, q1, f"block {block}", block=block)
    rows, _ = run_bank(hip, bank, ptr(d), 0, total, 1000, 3001)
    check_rows(hip, names, rows, ptr(d), 0, 1000, 3001, f"block {block}, outputs [1000,3001)", block=block)


def test_seam_blocks_the_banked_launch_refuses(hip):
    """A block of 100 samples is shorter than the decimator's 128 taps: no bank can be created with it (Filter.hs:544), so there
    is no run to refuse.  160 is the shortest kind of block a bank takes and the banked launch does not (its range starts at 192):
    route 1 refuses with nothing written, auto goes station by station, same bits."""
    names = ["shift -3/1000", "shift 1/4"]
    with pytest.raises(hip.SdrHipError):
        _bank(hip, names, 100)
    block = 160
    total = 20 * B
    d = dev()
    bank = _bank(hip, names, block)
    q0, q1, _ = bank.plan(0, total, total)
    b0 = hip.fm_bank_launches()
    bank.set_route(1)
    out = dev_empty_f32(2 * (q1 - q0))
    wsb = bank.workspace_bytes(total)
    ws = torch.empty(wsb, dtype=torch.uint8, device="cuda")
    rc = hip.lib.sdrhip_fm_bank_run_i16(bank.h, None, ptr(d), 0, total, ptr(out), q1 - q0, q0, q1, ptr(ws), wsb)
    assert rc == -1 and b"banked launch does not fit" in hip.lib.sdrhip_last_error()
    assert (to_host(out).view(np.uint32) == CANARY).all(), "a refused run wrote audio"
    bank.set_route(0)
    rows, _ = run_bank(hip, bank, ptr(d), 0, total, q0, q1)
    assert hip.fm_bank_launches() == b0, "block 160: no banked launch"
    check_rows(hip, names, rows, ptr(d), 0, q0, q1, "block 160, auto", block=block)


# ---- 7 ---------------------------------------------------------------------------------------------------------------------------
def test_alignment(hip):
    names = ["shift -3/1000", "shift 5/8313", "identity"]
    total = 12 * B
    d, d1 = dev(), dev("plus1")
    bank = _bank(hip, names)
    q0, q1, _ = bank.plan(0, total, total)
    n = q1 - q0
    # 16 bytes on: the buffer starts at stream sample 4, a multiple of 4 and not of 8
    Q0, Q1, _ = bank.plan(4, total, total)
    bank.set_route(1)
    b0 = hip.fm_bank_i16_launches()
    rows, _ = run_bank(hip, bank, ptr(d) + 16, 4, total - 4, Q0, Q1)
    assert hip.fm_bank_i16_launches() == b0 + 1
    check_rows(hip, names, rows, ptr(d), 0, Q0, Q1, "d_in 16 bytes on, s0 = 4")
    # 4 bytes past a 16-byte boundary
    p4 = ptr(d1) + 4
    assert p4 % 16 == 4
    b0 = hip.fm_bank_launches()
    out = dev_empty_f32(3 * n)
    wsb = bank.workspace_bytes(total)
    ws = torch.empty(wsb, dtype=torch.uint8, device="cuda")
    rc = hip.lib.sdrhip_fm_bank_run_i16(bank.h, None, p4, 0, total, ptr(out), n, q0, q1, ptr(ws), wsb)
    assert rc == -1 and (to_host(out).view(np.uint32) == CANARY).all(), "route 1 on input 4 bytes past a 16-byte boundary"
    bank.set_route(0)
    rows, _ = run_bank(hip, bank, p4, 0, total, q0, q1)
    assert hip.fm_bank_launches() == b0, "auto took the banked launch on input it cannot load"
    check_rows(hip, names, rows, ptr(d), 0, q0, q1, "4 bytes past a 16-byte boundary, auto")
    # 2 bytes past a 4-byte boundary: no route
    for route in (0, 1, 2):
        bank.set_route(route)
        out = dev_empty_f32(3 * n)
        rc = hip.lib.sdrhip_fm_bank_run_i16(bank.h, None, ptr(d) + 2, 0, total - 1, ptr(out), n, q0, q1 - 100, ptr(ws), wsb)
        assert rc == -1 and b"multiple of 4" in hip.lib.sdrhip_last_error(), route
        assert (to_host(out).view(np.uint32) == CANARY).all(), route
    assert hip.fm_bank_launches() == b0


# ---- 8 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 3, 32])
def test_route_2_equals_route_1(hip, K):
    """... on aligned input (the tuner's int16 tile kernel is every station's first stage) and on input 4 bytes past a 16-byte
    boundary, where the fused tuner refuses the first window and the first stage is the int16 mix and the cfloat decimator."""
    names = [FC.NAMES[(3 * j + 1) % len(FC.NAMES)] for j in range(K)]
    total = 12 * B
    d, d1 = dev(), dev("plus1")
    bank = _bank(hip, names)
    q0, q1, _ = bank.plan(0, total, total)
    bank.set_route(1)
    banked, _ = run_bank(hip, bank, ptr(d), 0, total, q0, q1)
    bank.set_route(2)
    c0 = counters(hip)
    rows, _ = run_bank(hip, bank, ptr(d), 0, total, q0, q1)
    c1 = counters(hip)
    assert c1[:3] == c0[:3] and c1[3] == c0[3] + K, "route 2, aligned: K launches of the tuner's int16 tile kernel, no one-kernel chain"
    assert_bit_equal(rows, banked, "route 2 vs route 1")
    rows, _ = run_bank(hip, bank, ptr(d1) + 4, 0, total, q0, q1)
    c2 = counters(hip)
    assert c2 == c1, "route 2 on a first window the fused tuner refuses: the two-pass mix, no tile kernel"
    assert_bit_equal(rows, banked, "route 2 (two-pass first stage) vs route 1")
    if K == 3:
        check_rows(hip, names, rows, ptr(d), 0, q0, q1, "route 2")


def test_auto_on_both_sides_of_its_edges(hip):
    names = ["shift -3/1000", "shift 1/4"]
    d = dev("long")
    total = 140 * B
    bank = _bank(hip, names)
    _, q1, _ = bank.plan(0, total, total)
    edge = 39322
    assert q1 > edge + 1
    n = 3000
    for max_outputs, banked in ((2 * n - 1, False), (2 * n, True)):
        bank.set_route(0, max_outputs)
        b0 = hip.fm_bank_i16_launches()
        rows, _ = run_bank(hip, bank, ptr(d), 0, total, 100, 100 + n)
        assert hip.fm_bank_i16_launches() == b0 + int(banked), max_outputs
        check_rows(hip, names, rows, ptr(d), 0, 100, 100 + n, f"max_outputs {max_outputs}", key="long")
    for max_outputs in (0, 2 ** 40):
        bank.set_route(0, max_outputs)
        for nq, banked in ((edge, True), (edge + 1, False)):
            b0 = hip.fm_bank_i16_launches()
            rows, _ = run_bank(hip, bank, ptr(d), 0, total, 0, nq)
            assert hip.fm_bank_i16_launches() == b0 + int(banked), (max_outputs, nq)
            check_rows(hip, names, rows, ptr(d), 0, 0, nq, f"{nq} outputs per station", key="long")


# ---- 9 ---------------------------------------------------------------------------------------------------------------------------
def test_subnormal_table(hip):
    names = ["subnormals", "shift 1/4"]
    total = 20 * B
    d = dev()
    bank = _bank(hip, names)
    for route in (1, 2):
        bank.set_route(route)
        rows, _ = run_bank(hip, bank, ptr(d), 0, total, 158, 4251)
        check_rows(hip, names, rows, ptr(d), 0, 158, 4251, f"route {route}")


def test_overflow_table_walks_the_padded_tap(hip, oracle):
    """fm_bank_i16_cases' overflow case: the table passes the chain's predicate and fails the int16 one, so the int16 launch must be
    the PSKIP = 0 form.  Checked by result: the NaN positions are the model's (tests/test_fm_bank_i16_cases.py shows that one of
    them is gone when the padded tap is skipped).  The u8 run of the same bank on a u8 stream still matches its own tuned chain."""
    names = ["overflow", "shift 1/4"]
    q0, q1 = FC.OVERFLOW_RANGE
    total = FC.OV_NBLK * B
    d = dev()
    exp = FC.model(oracle, "overflow", FC.OV_NBLK)[q0:q1]
    assert np.isnan(exp).any()
    bank = _bank(hip, names)
    for route in (1, 2):
        bank.set_route(route)
        b0 = hip.fm_bank_i16_launches()
        rows, _ = run_bank(hip, bank, ptr(d), 0, total, q0, q1)
        assert hip.fm_bank_i16_launches() == b0 + (route == 1)
        same_bits(rows[0], exp, f"route {route}: the overflow station vs the restated Pipes")
        check_rows(hip, names, rows, ptr(d), 0, q0, q1, f"route {route}")
    # u8 input: |x| <= 1, nothing overflows, the bank's u8 launch is its chain's
    u8 = T.stream_dev()
    bank.set_route(1)
    out = dev_empty_f32(2 * (q1 - q0))
    bank.run(ptr(u8), 0, total, ptr(out), q1 - q0, q0, q1)
    got = to_host(out).reshape(2, -1)
    for j, name in enumerate(names):
        ch = T._chain(hip, FC.table(name))
        T._route(ch, "small")
        assert_bit_equal(got[j], T._run(hip, ch, u8, 0, total, q0, q1), f"u8 run, station {j} vs its tuned chain")


# ---- 10 --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", [1, 2])
@pytest.mark.parametrize("gap", [0, 1, 5])
def test_memory_discipline(hip, route, gap):
    names = ["subnormals", "shift 1/4", "shift -3/1000"]
    total = 20 * B
    d = dev()
    bank = _bank(hip, names)
    q0, q1 = 158, 4251
    n, stride = q1 - q0, q1 - q0 + gap
    bank.set_route(route)
    rows, whole = run_bank(hip, bank, ptr(d), 0, total, q0, q1, stride=stride, workspace=(route == 2))
    gaps = whole.reshape(3, stride)[:, n:]
    assert (gaps == CANARY).all(), f"route {route}: floats between the rows were written"
    check_rows(hip, names, rows, ptr(d), 0, q0, q1, f"route {route}, rows {stride} floats apart")


def test_workspace_one_byte_short(hip):
    """Route 2 needs the stage routes' workspace for this run (chain.cpp's plan_run: decimated, demodulated and resampled ranges,
    each rounded up to 256 bytes; the tuner's tile kernel stages nothing): one byte less is refused with nothing written, the
    exact size runs."""
    names = ["shift 1/4", "shift -3/1000"]
    total = 20 * B
    d = dev()
    bank = _bank(hip, names)
    q0, q1 = 158, 4251
    r = FC.ranges(q0, q1)
    up = lambda b: (b + 255) // 256 * 256
    need = up(8 * (r["kd1"] - r["kd0"])) + up(4 * (r["ky1"] - r["ky0"])) + up(4 * (r["m1"] - q0))
    assert need <= bank.workspace_bytes(total)
    bank.set_route(2)
    out = dev_empty_f32(2 * (q1 - q0))
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    assert ptr(ws) % 256 == 0
    rc = hip.lib.sdrhip_fm_bank_run_i16(bank.h, None, ptr(d), 0, total, ptr(out), q1 - q0, q0, q1, ptr(ws), need - 1)
    assert rc == -1 and b"workspace" in hip.lib.sdrhip_last_error()
    assert (to_host(out).view(np.uint32) == CANARY).all(), "a refused run wrote audio"
    rows, _ = run_bank(hip, bank, ptr(d), 0, total, q0, q1, ws_bytes=need)
    check_rows(hip, names, rows, ptr(d), 0, q0, q1, "the exact workspace")
