"""GPU parity of the receiver bank (sdrhip_fm_bank_*): every station of one capture, one launch of the tuned one-kernel chain with a
station axis in its grid.  The definition is the whole specification: station j's row is, bit for bit, what a tuned FmChain of the
same arguments with table j writes for the same (s0, n_in, q0, q1), on every route of the bank and for any tile size.  Every
comparison here is against such chains run on the same device, or against the restated Pipes with the oscillator stage
(tests/tuned_chain_model.py) -- never against the bank itself.  Chain, stream, tables and the cached model are those of
tests/test_gpu_tuned_chain.py: /8 with 127 taps, 3/10 with 191 taps, 64 half taps, gain 0.2."""
import numpy as np
import pytest
import torch

import signals as S
import test_gpu_tuned_chain as T
from conftest import assert_bit_equal
from gpu_util import CANARY, dev_empty_f32, ptr, to_dev, to_host

pytestmark = pytest.mark.gpu

B = T.B
NAMES = list(T.TABLES) + ["subnormals", "identity"]          # periods 4, 1000, 8313, 5, 65536, 7, 1
_refs = {}


def tab(name):
    return {"subnormals": T.SUBNORMALS, "identity": T.IDENTITY}[name] if name in ("subnormals", "identity") else T.table(name)


def _bank(hip, names, block=B, decim_taps=None):
    return hip.FmBank(8, S.taps_decim127() if decim_taps is None else decim_taps, 3, 10, S.taps_resamp191(), S.taps_audio_half64(),
                      [tab(n) for n in names], T.GAIN, block)


def _chain(hip, name, block=B, decim_taps=None):
    ch = hip.FmChain(8, S.taps_decim127() if decim_taps is None else decim_taps, 3, 10, S.taps_resamp191(), S.taps_audio_half64(), T.GAIN, block)
    ch.set_tuner(tab(name))
    return ch


def chain_ref(hip, name, d_in, s0, n_in, q0, q1, block=B, route="small", decim_taps=None, key=None):
    """What the definition names: a tuned chain of the same arguments on the same run (computed once per run and table, never
    written).  key: what tells the input apart (default: the stream's prefix)."""
    k = (name, block, route, s0, n_in, q0, q1, decim_taps is not None, key)
    if k not in _refs:
        ch = _chain(hip, name, block, decim_taps)
        T._route(ch, route)
        c0 = hip.small_chain_tuned_launches()
        out = T._run(hip, ch, d_in, s0, n_in, q0, q1)
        if route == "small":
            assert hip.small_chain_tuned_launches() == c0 + 1, "the reference chain did not take its own one-kernel route"
        out.setflags(write=False)
        _refs[k] = out
    return _refs[k]


def run_bank(hip, bank, d_in, s0, n_in, q0, q1, stride=None, workspace=True):
    """-> (rows [stations, q1 - q0], the whole output buffer [stations * stride] as uint32)"""
    K, n = bank.stations(), q1 - q0
    stride = n if stride is None else stride
    out = dev_empty_f32(K * stride)
    ws_bytes = bank.workspace_bytes(n_in) if workspace else 0
    ws = torch.empty(max(ws_bytes, 16), dtype=torch.uint8, device="cuda") if workspace else None
    bank.run(ptr(d_in), s0, n_in, ptr(out), stride, q0, q1, ptr(ws) if workspace else None, ws_bytes)
    whole = to_host(out)                                       # checks the guard bands around the buffer
    return whole.reshape(K, stride)[:, :n], whole.view(np.uint32)


def check_rows(hip, names, rows, d_in, s0, n_in, q0, q1, what, **kw):
    assert rows.shape == (len(names), q1 - q0)
    for j, name in enumerate(names):
        assert_bit_equal(rows[j], chain_ref(hip, name, d_in, s0, n_in, q0, q1, **kw), f"{what}: station {j} ({name}) vs its tuned chain")


# ---- 1 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 3, 32])
def test_banked_route_equals_tuned_chains(hip, K):
    """20 source blocks from the stream's start.  Mixed periods; 3 stations: the first and the last share a table; 32: every table
    of the set four or five times over.  One banked launch per run, and none of the chains' own."""
    names = {1: ["shift 1/65536"], 3: ["shift -3/1000", "shift 5/8313", "shift -3/1000"], 32: [NAMES[j % len(NAMES)] for j in range(32)]}[K]
    total = 20 * B
    d = T.stream_dev()
    bank = _bank(hip, names)
    assert bank.stations() == K and [bank.period(j) for j in range(K)] == [tab(n).size // 2 for n in names]
    q0, q1, halo = bank.plan(0, total, total)
    decimated = (total - 128) // 8 + 1
    assert q0 == 0 and halo == 0 and q1 == (decimated * 3 - 192) // 10 + 1 - 127 == 5994      # as test_abi.py::test_chain_planning_on_the_host
    bank.set_route(1)
    for rep in range(2):
        b0, c0 = hip.fm_bank_launches(), hip.lib.sdrhip_debug_small_chain_launches()
        rows, _ = run_bank(hip, bank, d, 0, total, q0, q1, workspace=False)
        assert hip.fm_bank_launches() == b0 + 1, "one banked launch per run"
        assert hip.lib.sdrhip_debug_small_chain_launches() == c0, "a banked run launched a chain's kernel"
        check_rows(hip, names, rows, d, 0, total, q0, q1, f"{K} stations, run {rep}")
    if K == 3:
        assert not np.array_equal(rows[0], rows[1]), "two stations with different tables gave the same audio"


# ---- 2 ---------------------------------------------------------------------------------------------------------------------------
def test_against_the_restated_pipes(hip, oracle):
    """2 stations on 90 blocks (2 audio blocks each) against TCM.fm_receiver_tuned."""
    names = ["shift 1/4", "shift -3/1000"]
    total = 90 * B
    bank = _bank(hip, names)
    q0, q1, _ = bank.plan(0, total, total)
    assert q0 == 0 and q1 >= 2 * B
    bank.set_route(1)
    b0 = hip.fm_bank_launches()
    rows, _ = run_bank(hip, bank, T.stream_dev(), 0, total, 0, q1)
    assert hip.fm_bank_launches() == b0 + 1
    for j, name in enumerate(names):
        exp = T.model(oracle, name)
        assert exp.size == 2 * B
        assert_bit_equal(rows[j][:exp.size], exp, f"station {j} ({name}) vs the restated Pipes")


# ---- 3 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("q0,q1", [(1000, 3001), (0, 2000), (500, 501), (158, 158 + 4093)])
def test_edges_of_a_launch(hip, q0, q1):
    """q0 that starts no polyphase cycle, q1 inside a tile, a run of one output; tiles of 3, 96 and 159 outputs and the tile the
    launch picks itself: the same bits."""
    names = ["shift -3/1000", "random, period 5", "shift 5/8313"]
    total = 20 * B
    d = T.stream_dev()
    bank = _bank(hip, names)
    assert q0 % 3 != 0 or q0 == 0
    assert (q1 - q0 // 3 * 3) % 96 != 0 and (q1 - q0 // 3 * 3) % 159 != 0, "the run ends inside a tile"
    for tile in (0, 3, 96, 159):
        bank.set_route(1, 0, tile)
        b0 = hip.fm_bank_launches()
        rows, _ = run_bank(hip, bank, d, 0, total, q0, q1)
        assert hip.fm_bank_launches() == b0 + 1
        check_rows(hip, names, rows, d, 0, total, q0, q1, f"outputs [{q0},{q1}), tile of {tile}")


# ---- 4 ---------------------------------------------------------------------------------------------------------------------------
def test_far_stream_position(hip):
    """s0 = 2^33 + 8 * 12345 with periods 1000 and 65536: each station's launch phase is a 64-bit reduction of its own.  The buffer
    holds only the run's 6 blocks.  Then the same stream as three consecutive runs (each with its right halo)."""
    s0 = 2 ** 33 + 8 * 12345
    assert s0 % 8 == 0 and s0 % 1000 != 0 and s0 % 65536 != 0 and (s0 % 1000) != (s0 % 65536)
    n_in = 6 * B
    names = ["shift -3/1000", "shift 1/65536"]
    d = to_dev(T.stream_u8(6))
    bank = _bank(hip, names)
    end = s0 + n_in
    Q0, Q1, halo = bank.plan(s0, end, end)
    assert halo == 0 and Q1 - Q0 > 1500 and Q0 > 2 ** 28
    bank.set_route(1)
    b0 = hip.fm_bank_launches()
    full, _ = run_bank(hip, bank, d, s0, n_in, Q0, Q1)
    assert hip.fm_bank_launches() == b0 + 1
    check_rows(hip, names, full, d, s0, n_in, Q0, Q1, "far position", key="far")
    # the position reached every oscillator: the same samples at the stream's start give other audio
    near, _ = run_bank(hip, bank, d, 0, n_in, *bank.plan(0, n_in, n_in)[:2])
    for j in range(2):
        assert not np.array_equal(near[j][:1000], full[j][:1000])
    cut = (n_in // 3 // 8 - 1) * 8
    assert cut % 1000 != 0 and cut % 8 == 0
    pieces, prev = [], Q0
    for r in range(3):
        a = s0 + r * cut
        b = end if r == 2 else s0 + (r + 1) * cut
        q0, q1, halo = bank.plan(a, b, end)
        assert q0 == prev and halo <= bank.max_halo() and q1 > q0
        prev = q1
        piece = d[2 * (a - s0):]
        assert ptr(piece) % 16 == 0
        pieces.append(run_bank(hip, bank, piece, a, min(end, b + halo) - a, q0, q1)[0])
    assert prev == Q1 and hip.fm_bank_launches() == b0 + 5
    assert_bit_equal(np.concatenate(pieces, axis=1), full, "three consecutive runs vs one run")


# ---- 5 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("block", [0, 192, B])
def test_seams(hip, block):
    """Contiguous, the shortest seam block the kernel takes (a tile then meets 43 buffer boundaries) and the receiver's own."""
    names = ["shift -3/1000", "shift 1/4", "random, period 5"]
    total = 20 * B
    d = T.stream_dev()
    bank = _bank(hip, names, block)
    q0, q1, _ = bank.plan(0, total, total)
    bank.set_route(1)
    b0 = hip.fm_bank_launches()
    rows, _ = run_bank(hip, bank, d, 0, total, q0, q1)
    assert hip.fm_bank_launches() == b0 + 1
    check_rows(hip, names, rows, d, 0, total, q0, q1, f"block {block}", block=block)
    rows, _ = run_bank(hip, bank, d, 0, total, 1000, 3001)
    check_rows(hip, names, rows, d, 0, total, 1000, 3001, f"block {block}, outputs [1000,3001)", block=block)


def test_seam_blocks_the_banked_launch_refuses(hip):
    """A block of 100 samples is shorter than the decimator's 128 taps: no chain takes it (Filter.hs:544) and no bank does.  160
    is the chain's own case of a seam block below the one-kernel chain's range (test_gpu_tuned_chain.py::test_routes_are_bit_equal):
    forced, the banked route is an error; auto goes station by station."""
    names = ["shift -3/1000", "shift 1/4"]
    with pytest.raises(hip.SdrHipError):
        _chain(hip, names[0], 100)
    with pytest.raises(hip.SdrHipError):
        _bank(hip, names, 100)
    block = 160
    total = 20 * B
    d = T.stream_dev()
    bank = _bank(hip, names, block)
    q0, q1, _ = bank.plan(0, total, total)
    b0 = hip.fm_bank_launches()
    bank.set_route(1)
    out = dev_empty_f32(2 * (q1 - q0))
    wsb = bank.workspace_bytes(total)
    ws = torch.empty(wsb, dtype=torch.uint8, device="cuda")
    rc = hip.lib.sdrhip_fm_bank_run(bank.h, None, ptr(d), 0, total, ptr(out), q1 - q0, q0, q1, ptr(ws), wsb)
    assert rc == -1 and b"sdrhip_fm_bank_run" in hip.lib.sdrhip_last_error()
    assert (to_host(out).view(np.uint32) == CANARY).all(), "a refused run wrote audio"
    bank.set_route(0)
    rows, _ = run_bank(hip, bank, d, 0, total, q0, q1)
    assert hip.fm_bank_launches() == b0, "block 160: no banked launch"
    check_rows(hip, names, rows, d, 0, total, q0, q1, "block 160, auto", block=block, route="stage")


# ---- 6 ---------------------------------------------------------------------------------------------------------------------------
def test_fallbacks_in_auto(hip):
    names = ["shift -3/1000", "shift 5/8313", "identity"]
    nblk = 12
    total = nblk * B
    d = T.stream_dev()
    bank = _bank(hip, names)
    q0, q1, _ = bank.plan(0, total, total)
    n = q1 - q0
    # input 2 bytes off a 16-byte boundary: no tile kernel can load it
    shifted = to_dev(np.concatenate([np.zeros(2, np.uint8), T.stream_u8(nblk)]))[2:]
    assert ptr(shifted) % 16 == 2
    b0 = hip.fm_bank_launches()
    rows, _ = run_bank(hip, bank, shifted, 0, total, q0, q1)
    assert hip.fm_bank_launches() == b0, "unaligned input took the banked launch"
    check_rows(hip, names, rows, d, 0, total, q0, q1, "unaligned input, auto")
    bank.set_route(1)
    with pytest.raises(hip.SdrHipError):
        run_bank(hip, bank, shifted, 0, total, q0, q1)
    # the auto rule counts stations * outputs
    bank.set_route(0, 3 * n - 1)
    rows, _ = run_bank(hip, bank, d, 0, total, q0, q1)
    assert hip.fm_bank_launches() == b0, "max_outputs below stations * outputs: station by station"
    check_rows(hip, names, rows, d, 0, total, q0, q1, "max_outputs 3 n - 1")
    bank.set_route(0, 3 * n)
    rows, _ = run_bank(hip, bank, d, 0, total, q0, q1)
    assert hip.fm_bank_launches() == b0 + 1, "max_outputs = stations * outputs: the banked launch"
    check_rows(hip, names, rows, d, 0, total, q0, q1, "max_outputs 3 n")
    bank.set_route(0)                                          # the built-in bound takes a 12-block run
    banked, _ = run_bank(hip, bank, d, 0, total, q0, q1)
    assert hip.fm_bank_launches() == b0 + 2
    bank.set_route(2)
    stations, _ = run_bank(hip, bank, d, 0, total, q0, q1)
    assert hip.fm_bank_launches() == b0 + 2
    assert_bit_equal(stations, banked, "station by station vs the banked launch")
    check_rows(hip, names, stations, d, 0, total, q0, q1, "route 2")


def test_auto_banks_no_long_run_of_a_station(hip):
    """The auto rule has two dimensions: stations * outputs <= max_outputs AND outputs per station <= 39322 (a run of 2^20 samples,
    the longest the sweep behind the rule measured).  One output more goes station by station although 2 * 39323 is far below the
    built-in total, 32 * 39322 -- and also under a max_outputs that would admit it.  Same bits on both sides of the edge."""
    names = ["shift -3/1000", "shift 1/4"]
    total = 140 * B
    d = T.stream_dev()
    bank = _bank(hip, names)
    _, q1, _ = bank.plan(0, total, total)
    edge = 39322
    assert q1 > edge + 1 and 2 * (edge + 1) < 32 * edge
    for max_outputs in (0, 2 ** 40):
        bank.set_route(0, max_outputs)
        b0 = hip.fm_bank_launches()
        rows, _ = run_bank(hip, bank, d, 0, total, 0, edge)
        assert hip.fm_bank_launches() == b0 + 1, f"{edge} outputs per station, max_outputs {max_outputs}: the banked launch"
        check_rows(hip, names, rows, d, 0, total, 0, edge, f"{edge} outputs per station")
        rows, _ = run_bank(hip, bank, d, 0, total, 0, edge + 1)
        assert hip.fm_bank_launches() == b0 + 1, f"{edge + 1} outputs per station, max_outputs {max_outputs}: station by station"
        check_rows(hip, names, rows, d, 0, total, 0, edge + 1, f"{edge + 1} outputs per station")
    bank.set_route(1)                                          # forced, the launch still takes the longer run
    b0 = hip.fm_bank_launches()
    rows, _ = run_bank(hip, bank, d, 0, total, 0, edge + 1)
    assert hip.fm_bank_launches() == b0 + 1
    check_rows(hip, names, rows, d, 0, total, 0, edge + 1, f"{edge + 1} outputs per station, route 1")


# ---- 7 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", [1, 2])
def test_memory_discipline(hip, route):
    """Rows 37 floats apart: the gaps (and the guard bands around the buffer, which to_host checks) keep their canaries.  Table 0
    is the subnormal / negative-zero table."""
    names = ["subnormals", "shift 1/4", "shift -3/1000"]
    total = 20 * B
    d = T.stream_dev()
    bank = _bank(hip, names)
    q0, q1 = 158, 158 + 4093
    n, stride = q1 - q0, q1 - q0 + 37
    bank.set_route(route)
    rows, whole = run_bank(hip, bank, d, 0, total, q0, q1, stride=stride)
    gaps = whole.reshape(3, stride)[:, n:]
    assert (gaps == CANARY).all(), f"route {route}: {int((gaps != CANARY).sum())} floats between the rows were written"
    check_rows(hip, names, rows, d, 0, total, q0, q1, f"route {route}, stride n + 37")


def test_launches_that_skip_no_tap(hip):
    """The launch walks all 128 taps (PSKIP = 0) when the last prepared tap is no padding (a 128-tap decimator) and when ANY
    station's mixed samples can overflow (|re| + |im| beyond FLT_MAX: finite entries, so a legal table) -- for every station of the
    launch, also those whose own chain skips the zero tap.  The bits are the chains' either way."""
    total = 6 * B
    d = T.stream_dev()
    taps128 = S.gauss_taps(128, 128128)
    names = ["random, period 5", "subnormals"]
    bank = _bank(hip, names, decim_taps=taps128)
    q0, q1, _ = bank.plan(0, total, total)
    bank.set_route(1)
    rows, _ = run_bank(hip, bank, d, 0, total, q0, q1)
    check_rows(hip, names, rows, d, 0, total, q0, q1, "128-tap decimator", decim_taps=taps128)
    huge = np.array([3e38, 3e38, 1.0, 0.0, -3e38, 2e38], np.float32)
    ch = _chain(hip, "identity")
    ch.set_tuner(huge)
    T._route(ch, "small")
    exp = T._run(hip, ch, d, 0, total, q0, q1)
    bank = hip.FmBank(8, S.taps_decim127(), 3, 10, S.taps_resamp191(), S.taps_audio_half64(), [huge, tab("shift 1/4")], T.GAIN, B)
    bank.set_route(1)
    rows, _ = run_bank(hip, bank, d, 0, total, q0, q1)
    assert_bit_equal(rows[0], exp, "a table whose mixed samples overflow vs its tuned chain")
    assert_bit_equal(rows[1], chain_ref(hip, "shift 1/4", d, 0, total, q0, q1), "its neighbour in the same launch vs its tuned chain")


# ---- 8 ---------------------------------------------------------------------------------------------------------------------------
def test_argument_errors_on_the_device_path(hip):
    names = ["shift -3/1000", "shift 1/4"]
    nblk = 12
    total = nblk * B
    d = T.stream_dev()
    bank = _bank(hip, names)
    q0, q1, _ = bank.plan(0, total, total)
    n = q1 - q0
    wsb = bank.workspace_bytes(total)
    ws = torch.empty(wsb, dtype=torch.uint8, device="cuda")
    run = hip.lib.sdrhip_fm_bank_run
    b0 = hip.fm_bank_launches()

    def untouched(out, what):
        assert (to_host(out).view(np.uint32) == CANARY).all(), what + ": a refused run wrote audio"

    for route in (0, 1, 2):
        bank.set_route(route)
        out = dev_empty_f32(2 * n)
        assert run(bank.h, None, ptr(d), 0, total, ptr(out), n - 1, q0, q1, ptr(ws), wsb) == -1, route       # rows would overlap
        assert b"sdrhip_fm_bank_run" in hip.lib.sdrhip_last_error()
        untouched(out, f"route {route}, audio_stride n - 1")
        # outputs whose receptive field the buffer does not hold
        assert run(bank.h, None, ptr(d), 0, total - B, ptr(out), n, q0, q1, ptr(ws), wsb) == -1, route
        untouched(out, f"route {route}, short input")
    # a workspace too small for the station-by-station route: unaligned input sends every station to the stage kernels
    shifted = to_dev(np.concatenate([np.zeros(2, np.uint8), T.stream_u8(nblk)]))[2:]
    for route in (0, 2):
        bank.set_route(route)
        out = dev_empty_f32(2 * n)
        assert run(bank.h, None, ptr(shifted), 0, total, ptr(out), n, q0, q1, ptr(ws), 4096) == -1, route
        assert b"workspace" in hip.lib.sdrhip_last_error()
        untouched(out, f"route {route}, workspace of 4096 bytes")
        assert run(bank.h, None, ptr(shifted), 0, total, ptr(out), n, q0, q1, None, 0) == -1, route
        untouched(out, f"route {route}, no workspace")
    assert hip.fm_bank_launches() == b0
    # the banked route sends nothing through the workspace
    bank.set_route(1)
    rows, _ = run_bank(hip, bank, d, 0, total, q0, q1, workspace=False)
    assert hip.fm_bank_launches() == b0 + 1
    check_rows(hip, names, rows, d, 0, total, q0, q1, "no workspace")
