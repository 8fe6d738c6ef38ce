"""The saved state of every Pipe kind, byte for byte (sdrhip_pipe_state_bytes / _save / _restore, sdr_amd/csrc/pipes_state.cpp).

One small deterministic scenario or more per kind, so that every record of the layout and every option is written at least once.  Each
pushes a seeded sequence with blocks of other sizes in it (the ragged path, all_uniform = 0), pops HALF of the blocks that are ready (a
fifo that is not empty), and saves where a carried tail -- and, for the rows-tail kinds, carried rows (y_n > 0) -- exist.

  * length and sha256 of the saved bytes are those recorded in tests/golden/pipe_state_digests.json, which a build of the commit named
    in that file wrote on an MI355X (python tests/test_gpu_pipe_state_bytes.py --record FILE --parent HASH, twice in separate
    processes, the two files equal); sdrhip_pipe_state_bytes gave that length;
  * a fresh pipe restored from the bytes saves the same bytes again and, pushed the rest of the sequence, yields bit for bit what the
    uninterrupted pipe yields;
  * the record sizes of the documented layout, restated here from the header fields of the saved bytes alone, sum to the length;
  * the state cut one byte short of each record boundary and of its end is refused as a `truncated state`, and the same pipe object
    then takes the whole state and goes on bit for bit: the refusals left it fresh.

The layout (versions 1 and 2): header (112 bytes) | rows record (8, version 2 only) | history (hist_n elements) | fifo (K * pending
floats) | n_blocks int32 | bank record (AM and NFM kinds: 8 + n_floats floats) | audio record (32 + K * y_n floats) | narrow record
(48 + n_floats floats + K * y_n * 2 floats).  Version 3 (the waterfall): its header (88 bytes) | tail_n samples | pending floats."""
import ctypes as C
import hashlib
import json
import os
import struct
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(HERE))

import narrow_bank_cases as NB
import pipe_am_bank_cases as PC
import signals as S
import tuner_model as TM

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(HERE, "golden", "pipe_state_digests.json")
BEFORE = [1024, 1024, 777, 1024, 1024, 1500]          # pushed before the save: one odd block, one longer one
AFTER = [1024, 600, 1024, 1024]                       # ... and behind it
TOTAL = sum(BEFORE) + sum(AFTER)
KIND = {"filter": 0, "decimator": 1, "resampler": 2, "fm_demod": 3, "dc_blocker": 4, "agc": 5, "tuner": 6, "tuner_bank": 7, "am_demod": 8,
        "am_bank": 9, "spectrum": 10, "nfm_bank": 11, "am_bank_audio": 12, "nfm_bank_audio": 13, "narrow_bank": 14}
MAP_KINDS = ("fm_demod", "am_demod", "dc_blocker", "agc")
BANK_RECORD = (9, 11, 12, 13)
AUDIO_RECORD = (12, 13)


def _tables():
    return [TM.shift_table(1, 4), TM.shift_table(-3, 1000)]


def _bank(hip):
    return hip.TunerBank(8, S.taps_decim51(), _tables())


def _fmt(fmt):
    return dict(input_u8=fmt == "u8", input_i16=fmt == "i16")


def _tail(hip):
    return hip.AudioTail(3, 10, S.taps_resamp31(), S.taps_audio_half32(), gain=-0.5, block=64)


def _narrow(hip, form, dc):
    return hip.NarrowBank(_bank(hip), hip.Decimator(4, NB.SHAPES["24/4"][0], complex_=True), form, dc)


def _spectrum(hip, fmt, n):
    return hip.Spectrum(n, {"u8": hip.IQ_U8, "cf32": hip.IQ_CF32, "i16": hip.IQ_I16}[fmt], hip.WINDOW_HANNING, True, 1.0 / n)


# name: (kind, what a block is, make(hip) -> Pipe[, (sizes before the save, sizes behind it)])
SCENARIOS = {
    "filter real": ("filter", "real", lambda hip: hip.Pipe("filter", hip.Filter(S.gauss_taps(32, 9)), 100)),
    "filter complex": ("filter", "cf32", lambda hip: hip.Pipe("filter", hip.Filter(S.gauss_taps(32, 9), complex_=True), 100)),
    "decimator real": ("decimator", "real", lambda hip: hip.Pipe("decimator", hip.Decimator(4, S.taps_decim51()), 100)),
    "decimator complex": ("decimator", "cf32", lambda hip: hip.Pipe("decimator", hip.Decimator(8, S.taps_decim51(), complex_=True), 100)),
    "resampler real 3/10": ("resampler", "real", lambda hip: hip.Pipe("resampler", hip.Resampler(3, 10, S.taps_resamp31()), 100)),
    "resampler complex 3/10": ("resampler", "cf32", lambda hip: hip.Pipe("resampler", hip.Resampler(3, 10, S.taps_resamp31(), complex_=True), 100)),
    "fmDemod": ("fm_demod", "cf32", lambda hip: hip.Pipe("fm_demod")),
    "amDemod": ("am_demod", "cf32", lambda hip: hip.Pipe.am_demod()),
    "dcBlocker": ("dc_blocker", "real", lambda hip: hip.Pipe("dc_blocker")),
    "agc": ("agc", "cf32", lambda hip: hip.Pipe("agc", mu=0.01, reference=0.5)),
    "tuner": ("tuner", "cf32", lambda hip: hip.Pipe.tuner(hip.Tuner(8, S.taps_decim51(), _tables()[0]), 100)),
    "tuner bank cfloat": ("tuner_bank", "cf32", lambda hip: hip.Pipe.tuner_bank(_bank(hip), 100)),
    "tuner bank u8": ("tuner_bank", "u8", lambda hip: hip.Pipe.tuner_bank(_bank(hip), 100, input_u8=True)),
    "tuner bank int16": ("tuner_bank", "i16", lambda hip: hip.Pipe.tuner_bank(_bank(hip), 100, input_i16=True)),
    "AM bank dc_block": ("am_bank", "u8", lambda hip: hip.Pipe.am_bank(hip.AmBank(_bank(hip), dc_block=True), 100, **_fmt("u8"))),
    "AM bank": ("am_bank", "i16", lambda hip: hip.Pipe.am_bank(hip.AmBank(_bank(hip), dc_block=False), 100, **_fmt("i16"))),
    "NFM bank": ("nfm_bank", "cf32", lambda hip: hip.Pipe.nfm_bank(hip.NfmBank(_bank(hip)), 100)),
    "AM bank audio": ("am_bank_audio", "i16", lambda hip: hip.Pipe.am_bank_audio(hip.AmBank(_bank(hip), dc_block=True), _tail(hip), **_fmt("i16"))),
    "NFM bank audio": ("nfm_bank_audio", "u8", lambda hip: hip.Pipe.nfm_bank_audio(hip.NfmBank(_bank(hip)), _tail(hip), **_fmt("u8"))),
    "narrow bank FM": ("narrow_bank", "u8", lambda hip: hip.Pipe.narrow_bank(_narrow(hip, NB.FM, False), 100, 16, **_fmt("u8"))),
    "narrow bank envelope": ("narrow_bank", "cf32", lambda hip: hip.Pipe.narrow_bank(_narrow(hip, NB.ENV, False), 100, 16)),
    "narrow bank envelope dc_block": ("narrow_bank", "i16", lambda hip: hip.Pipe.narrow_bank(_narrow(hip, NB.ENV, True), 100, 16, **_fmt("i16"))),
    # n 64, hop 101, group 2: three rows need 569 samples and use 606, so 26 samples of the stream are still to be skipped at the save
    "waterfall hop > n": ("spectrum", "u8", lambda hip: hip.Pipe.spectrum(_spectrum(hip, "u8", 64), 101, 2, 1, 0, -120.0),
                          ([200, 150, 77, 153], [64, 300, 101])),
    # n 64, hop 32, group 3: four rows use 384 of the 500 samples, 116 are the carried tail
    "waterfall group 3": ("spectrum", "i16", lambda hip: hip.Pipe.spectrum(_spectrum(hip, "i16", 64), 32, 3, 0, 1, -120.0),
                          ([128, 128, 100, 144], [64, 300, 32])),
}
NAMES = list(SCENARIOS)


def blocks_of(name):
    """(blocks pushed before the save, blocks pushed behind it)"""
    sc = SCENARIOS[name]
    before, after = sc[3] if len(sc) > 3 else (BEFORE, AFTER)
    what = sc[1]
    s = PC.stream("cf32", TOTAL) if what == "real" else PC.stream(what, TOTAL)
    w = 1 if what == "real" else 2
    edges = np.concatenate([[0], np.cumsum(before + after)]) * w
    blocks = [np.ascontiguousarray(s[a:b]) for a, b in zip(edges[:-1], edges[1:])]
    return blocks[:len(before)], blocks[len(before):]


def raw_push(hip, p, blk):
    """One push that pops nothing: the count of ready blocks."""
    if p.input_u8:
        return hip.check(hip.lib.sdrhip_pipe_push_u8(p.h, blk.ctypes.data_as(C.POINTER(C.c_uint8)), blk.size // 2), "push_u8")
    if p.input_i16:
        return hip.check(hip.lib.sdrhip_pipe_push_i16(p.h, blk.ctypes.data_as(C.POINTER(C.c_int16)), blk.size // 2), "push_i16")
    return hip.check(hip.lib.sdrhip_pipe_push(p.h, blk.ctypes.data_as(C.POINTER(C.c_float)), blk.size // (2 if p.complex_in else 1)), "push")


def joined(outs):
    """What a pipe yielded as one array: the rows of a bank side by side, everything else end to end."""
    if not outs:
        return np.empty(0, np.float32)
    return np.concatenate(outs, axis=outs[0].ndim - 1)


def state_bytes(hip, p):
    hip.lib.sdrhip_pipe_state_bytes.restype = C.c_size_t
    hip.lib.sdrhip_pipe_state_bytes.argtypes = [C.c_void_p]
    return hip.lib.sdrhip_pipe_state_bytes(p.h)


def raw_restore(hip, p, state):
    hip.lib.sdrhip_pipe_restore.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t]
    return hip.lib.sdrhip_pipe_restore(p.h, state, len(state))


def fresh(hip, name):
    p = SCENARIOS[name][2](hip)
    p._cap = max(BEFORE + AFTER)            # the map Pipes hand blocks back at the length they came in
    return p


def play(hip, name):
    """The scenario up to its save -> (the saved pipe, state, what state_bytes said, blocks ready at the save, blocks popped before it)."""
    before, _ = blocks_of(name)
    a = fresh(hip, name)
    for blk in before:
        raw_push(hip, a, blk)
    ready = hip.check(hip.lib.sdrhip_pipe_flush(a.h), "flush")
    assert ready >= 2, f"{name}: {ready} blocks ready: the scenario must leave some in the fifo and pop some"
    a._pop(ready // 2)
    said = state_bytes(hip, a)
    return a, a.save(), said, ready - ready // 2


def rest_of(hip, name, p, ready):
    """Pop what is ready, push the rest of the sequence and flush -> everything the pipe yields from the save on."""
    _, after = blocks_of(name)
    outs = p._pop(ready)
    for blk in after:
        outs += p.push(blk)
    return joined(outs + p.flush())


_played = {}


def played(hip, name):
    """(state, what state_bytes said, the uninterrupted pipe's output from the save on), computed once and left unchanged"""
    if name not in _played:
        a, state, said, ready = play(hip, name)
        out = rest_of(hip, name, a, ready)
        out.setflags(write=False)
        _played[name] = (state, said, ready, out)
    return _played[name]


def same_bits(got, want, what):
    assert got.shape == want.shape and got.size > 0, f"{what}: {got.shape} against {want.shape}"
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), f"{what}: the outputs differ"


# ---- the documented layout, restated --------------------------------------------------------------------------------------------------
def records(state):
    """[(record, bytes)] of a saved state by the documented layout, from the header fields of the bytes alone."""
    magic, version, kind = struct.unpack_from("<IIi", state, 0)
    assert magic == 0x50504453
    if version == 3:
        n, input_type = struct.unpack_from("<ii", state, 12)
        tail_n, pending = struct.unpack_from("<qq", state, 72)
        return kind, [("header", 88), ("tail", tail_n * {0: 8, 1: 2, 2: 4}[input_type]), ("fifo", pending * 4)]
    cplx_in, = struct.unpack_from("<i", state, 28)
    n_blocks, = struct.unpack_from("<i", state, 44)
    hist_n, pending = struct.unpack_from("<qq", state, 72)
    recs = [("header", 112)]
    K, esz = 1, 4 * (2 if cplx_in else 1)
    if version == 2:
        K, input_type = struct.unpack_from("<ii", state, 112)
        esz = {0: esz, 1: 2, 2: 4}[input_type]
        recs.append(("rows", 8))
    recs += [("history", hist_n * esz), ("fifo", K * pending * 4), ("blocks", n_blocks * 4)]
    at = sum(b for _, b in recs)
    if kind in BANK_RECORD:
        n_floats, = struct.unpack_from("<i", state, at + 4)
        recs.append(("bank", 8 + n_floats * 4))
        at += 8 + n_floats * 4
    if kind in AUDIO_RECORD:
        y_n, = struct.unpack_from("<q", state, at + 8)
        assert y_n > 0, "the scenario must save carried rows"
        recs.append(("audio", 32 + K * y_n * 4))
    if kind == KIND["narrow_bank"]:
        y_n, = struct.unpack_from("<q", state, at + 8)
        n_floats, = struct.unpack_from("<i", state, at + 40)
        assert y_n > 0, "the scenario must save carried rows"
        recs.append(("narrow", 48 + n_floats * 4 + K * y_n * 8))
    return kind, recs


def cuts(state):
    """{cut length: which boundary}: one byte short of every record boundary and of the end"""
    _, recs = records(state)
    out, at = {}, 0
    for rec, b in recs:
        at += b
        if b:
            out.setdefault(at - 1, rec)
    return out


# ---- the tests ------------------------------------------------------------------------------------------------------------------------
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_every_kind_has_a_scenario_and_a_recorded_digest():
    assert {SCENARIOS[n][0] for n in NAMES} == set(KIND)
    g = golden()
    assert len(g["parent"]) == 40 and set(g["digests"]) == set(NAMES)


@pytest.mark.parametrize("name", NAMES)
def test_saved_bytes_are_the_parent_s(hip, name):
    state, said, _, _ = played(hip, name)
    want = golden()["digests"][name]
    print(f"{name}: {len(state)} bytes, sha256 {hashlib.sha256(state).hexdigest()}, state_bytes {said}")
    assert len(state) == want["bytes"], f"{name}: {len(state)} bytes saved, the parent saved {want['bytes']}"
    assert hashlib.sha256(state).hexdigest() == want["sha256"], f"{name}: the saved bytes changed"
    assert said == len(state), f"{name}: sdrhip_pipe_state_bytes said {said}"


@pytest.mark.parametrize("name", NAMES)
def test_the_restored_pipe_saves_the_same_and_goes_on_bit_for_bit(hip, name):
    state, _, ready, want = played(hip, name)
    b = fresh(hip, name)
    assert raw_restore(hip, b, state) == ready, hip.lib.sdrhip_last_error()
    assert state_bytes(hip, b) == len(state)
    again = b.save()
    assert hashlib.sha256(again).hexdigest() == hashlib.sha256(state).hexdigest(), f"{name}: the restored pipe saves other bytes"
    same_bits(rest_of(hip, name, b, ready), want, f"{name}: the restored pipe against the uninterrupted one")


@pytest.mark.parametrize("name", NAMES)
def test_the_records_of_the_layout_sum_to_the_length(hip, name):
    state = played(hip, name)[0]
    kind, recs = records(state)
    print(f"{name}: {recs}")
    assert kind == KIND[SCENARIOS[name][0]]
    assert sum(b for _, b in recs) == len(state), f"{name}: {recs} against {len(state)} bytes"
    sizes = dict(recs)
    assert sizes["fifo"] > 0, f"{name}: an empty fifo"
    if name == "waterfall hop > n":
        assert struct.unpack_from("<q", state, 64)[0] > 0 and sizes["tail"] == 0, "skip is not live"
    elif kind == KIND["spectrum"]:
        assert sizes["tail"] > 0, f"{name}: no carried tail"
    elif SCENARIOS[name][0] in MAP_KINDS:
        assert sizes["blocks"] > 0 and sizes["history"] == 0, f"{name}: a map Pipe's state is its block lengths"
    else:
        assert sizes["history"] > 0 and sizes["blocks"] == 0, f"{name}: no carried tail"
        assert struct.unpack_from("<i", state, 40)[0] == 0, f"{name}: all_uniform is still set"


def truncation(hip, name, which):
    """The cuts `which` selects are refused as truncated, and the pipe that refused them then takes the whole state."""
    state, _, ready, want = played(hip, name)
    b = fresh(hip, name)
    todo = {n: rec for n, rec in cuts(state).items() if which(rec)}
    assert todo
    for n, rec in sorted(todo.items()):
        rc = raw_restore(hip, b, state[:n])
        msg = hip.lib.sdrhip_last_error().decode()
        print(f"{name}: {n} of {len(state)} bytes (one short of the end of `{rec}`): {rc}, {msg}")
        assert rc == -1 and "truncated state" in msg, f"{name}: cut one byte short of the end of `{rec}`: {rc}, {msg}"
        assert hip.lib.sdrhip_pipe_poll(b.h) == 0
    assert raw_restore(hip, b, state) == ready, hip.lib.sdrhip_last_error()
    same_bits(rest_of(hip, name, b, ready), want, f"{name}: the pipe that refused the cut states against the uninterrupted one")


@pytest.mark.parametrize("name", NAMES)
def test_a_state_cut_short_of_a_record_boundary_is_refused_and_leaves_the_pipe_fresh(hip, name):
    truncation(hip, name, lambda rec: rec != "header" or SCENARIOS[name][0] == "spectrum")


@pytest.mark.xfail(strict=True, reason="a version 1 / 2 state cut inside its 112-byte header is refused by the argument check in front of "
                   "every other one (`bytes >= sizeof(PipeStateHeader)`), whose text does not say `truncated state`: so on the parent "
                   "commit, and error texts are not this test's to change")
@pytest.mark.parametrize("name", ["filter real", "tuner bank u8"], ids=["version 1", "version 2"])
def test_a_state_cut_one_byte_short_of_its_header_is_refused_as_truncated(hip, name):
    truncation(hip, name, lambda rec: rec == "header")


if __name__ == "__main__":
    import argparse
    ap = argparse.ArgumentParser(description="record the scenarios' digests from the tree this file stands in")
    ap.add_argument("--record", required=True)
    ap.add_argument("--parent", required=True, help="hash of the commit whose build writes the digests")
    args = ap.parse_args()
    import sdr_amd.lib as hip
    digests = {}
    for name in NAMES:
        _, state, said, _ = play(hip, name)
        digests[name] = {"bytes": len(state), "sha256": hashlib.sha256(state).hexdigest()}
        assert said == len(state), (name, said, len(state))
    with open(args.record, "w") as f:
        json.dump({"parent": args.parent, "recorded_on": hip.device_name(), "digests": digests}, f, indent=1)
        f.write("\n")
    print(f"{len(digests)} digests -> {args.record}")
