"""The cases of the AM bank Pipe's tests (tests/test_pipe_am_bank_abi.py, tests/test_gpu_pipe_am_bank.py): streams in the three input
types, the model of every channel's audio -- the restated firDecimator Pipe (oracle/pipes_model.py) on the stream mixed with the
channel's table (tests/tuner_model.py) at the pushes' own block boundaries, then agc_model.magnitude, then the oracle's dcBlocker over
the whole stream; both are independent of the block sizes -- and the saved states of every Pipe kind that existed before the AM bank's.
TEST INFRASTRUCTURE ONLY."""
import numpy as np

import agc_model as AM
import signals as S
import test_gpu_tuner as T
import tuner_i16_cases as IC
import tuner_model as TM
from oracle import pipes_model as PM

B, LP, D = 8192, 128, 8
FORMATS = ("cf32", "u8", "i16")
_cache = {}


def stream(fmt, nsamples):
    """The samples as the pipe takes them: uint8 IQ, int16 IQ, or the u8 stream converted to float32 (exact)."""
    key = ("s", fmt, nsamples)
    if key not in _cache:
        if fmt == "i16":
            s = IC.stream_i16(nsamples, seed=1603)
        else:
            rng = np.random.default_rng(20241020)
            s = rng.integers(0, 256, 2 * nsamples, dtype=np.uint8)
            if fmt == "cf32":
                s = (s.astype(np.float32) - np.float32(128.0)) * np.float32(1.0 / 128.0)
            s.setflags(write=False)
        _cache[key] = s
    return _cache[key]


def converted(oracle, fmt, nsamples):
    s = stream(fmt, nsamples)
    return oracle.convert_i16(s) if fmt == "i16" else oracle.convert_u8(stream("u8", nsamples)) if fmt == "u8" else s


def cut(s, sizes):
    edges = np.concatenate([[0], np.cumsum(sizes)])
    assert edges[-1] * 2 <= s.size
    return [s[2 * a:2 * b] for a, b in zip(edges[:-1], edges[1:])]


def expected(oracle, table, fmt, sizes, dc, nsamples, taps=None, factor=8):
    """Channel audio of the whole stream pushed as blocks of `sizes`: every output that fills a block of 8 (block_size_out 1000 and
    1024 are multiples of 8, so every popped block lies inside).  -> float32, read-only."""
    taps = S.taps_decim127() if taps is None else taps
    key = ("e", np.asarray(table, np.float32).tobytes(), "i16" if fmt == "i16" else "u8", tuple(int(v) for v in sizes), nsamples, taps.tobytes(), factor)
    if key not in _cache:
        x = converted(oracle, fmt, nsamples)
        m = TM.mix(x, table)
        model = PM.FilterModel(oracle, taps, PM.ORDER_AVX, complex_=True, factor=factor)
        out, _ = PM.fir_decimator_pipe(model, cut(m, sizes), 8)
        iq = np.concatenate(out)
        env = AM.magnitude(iq[0::2], iq[1::2])
        audio = oracle.dc_blocker(env, 0.0, 0.0)[0]
        env.setflags(write=False)
        audio.setflags(write=False)
        _cache[key] = (env, audio)
    return _cache[key][1 if dc else 0]


def existing_kind_states(hip):
    """{kind: saved state} of every Pipe kind that existed before the AM bank's, each after three 8192-element pushes of one seeded
    stream, a flush and the pops: position, history, carried values and the outputs that fill no block yet.  Only calls that the
    parent tree has."""
    u8 = stream("u8", 3 * B)
    cf = stream("cf32", 3 * B)
    taps = S.taps_decim127()
    tabs = [T.osc_table(1000), np.array([1.0, 0.0], np.float32), T.osc_table(5)]
    pipes = {
        "filter": (hip.Pipe("filter", hip.Filter(S.gauss_taps(32, 9)), 1000), "real"),
        "decimator": (hip.Pipe("decimator", hip.Decimator(8, taps, hip.ORDER_AVX, complex_=True), 1000), "cplx"),
        "resampler": (hip.Pipe("resampler", hip.Resampler(3, 10, S.taps_resamp191()), 1000), "real"),
        "fm_demod": (hip.Pipe("fm_demod"), "cplx"),
        "dc_blocker": (hip.Pipe("dc_blocker"), "real"),
        "agc": (hip.Pipe("agc", mu=0.01, reference=0.5), "cplx"),
        "tuner": (hip.Pipe.tuner(hip.Tuner(8, taps, tabs[0]), 1000), "cplx"),
        "tuner_bank": (hip.Pipe.tuner_bank(hip.TunerBank(8, taps, tabs), 1000, input_u8=True), "u8"),
        "am_demod": (hip.Pipe.am_demod(), "cplx"),
    }
    states = {}
    for kind, (p, what) in pipes.items():
        if kind in ("filter", "decimator", "resampler", "tuner", "tuner_bank"):
            p.set_adaptive(0)
        for i in range(3):
            if what == "u8":
                p.push(u8[2 * B * i:2 * B * (i + 1)])
            elif what == "cplx":
                p.push(cf[2 * B * i:2 * B * (i + 1)])
            else:
                p.push(cf[B * i:B * (i + 1)])
        p.flush()
        states[kind] = p.save()
    return states


# sha256 of existing_kind_states(hip) with `hip` bound to a build of the PARENT commit's tree (its sdr_amd/lib.py over its
# libsdr_hip.so), printed on an MI355X by a throw-away script that imported this function
PARENT_STATE_SHA256 = {
    "filter": "3c61df07880a8feb002a3a0e81f9d8e466d751ef2da1fb06c08b41dbe23087a8",      # 2468 bytes
    "decimator": "120aa4eaea95a0c385f337c7031bb46d7a0d821fe2313fcca3221228f43fa9b7",      # 1752 bytes
    "resampler": "6a5449fa81ad4a6f1a0ddea6ee1a243dc8962e4276bf48da9c258b325cbf173f",      # 1832 bytes
    "fm_demod": "3a7b3969f7a844ad14ca3049b593d72638baddb49c98a9687c89bee418bffd0d",      # 112 bytes
    "dc_blocker": "2b73b127725c3dbc59aa139db73dc60c53b11f38b198ac89ed936aace82948a7",      # 112 bytes
    "agc": "e17ab3d1d3a1aa91d83d1b180be1385e36222c1f07a10663213442b734976b52",      # 112 bytes
    "tuner": "fb629a60a48551a8a150089c37c2876e797a622682582db5e664543e834122a9",      # 1752 bytes
    "tuner_bank": "62a34e7d53b01e45b7ff7a6d5029bd945e502e7ffc966d70de8e4efd280714df",      # 1808 bytes
    "am_demod": "af90a308b507743eedbb2d1298da3911a50a83f428ead1e552389227dadf610f",      # 112 bytes
}
