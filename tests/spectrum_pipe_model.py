"""The waterfall Pipe's bookkeeping (include/sdr_hip.h, sdrhip_pipe_spectrum) restated in Python, the int16 additions to the spectrum
models, and the cases its tests share.  With S every sample pushed so far, output row R exists as soon as
(R * group + group - 1) * hop + n <= |S|; the host keeps the samples from stream position rows_done * group * hop onward (the tail), or,
where that position lies beyond |S| (hop > n), the count of samples still to drop on arrival (the skip).  TEST INFRASTRUCTURE ONLY."""
import ctypes as C

import numpy as np

import spectrum_model as M
import tuner_i16_cases as IC

IQ_I16 = 2
SAMPLE_BYTES = {"u8": 2, "cf32": 8, "i16": 4}
TAIL_CAP_BYTES = 4 << 20


class PipeModel:
    """push(m) -> rows completed by this push; rows_done, tail and skip are the Pipe's state between pushes."""

    def __init__(self, n, hop, group):
        self.n, self.hop, self.group = n, hop, group
        self.pos = self.rows_done = self.tail = self.skip = 0

    def push(self, m):
        assert m >= 1
        drop = min(self.skip, m)
        self.skip -= drop
        self.pos += m
        have = self.tail + (m - drop)
        r = ((have - self.n) // self.hop + 1) // self.group if have >= self.n else 0
        used = r * self.group * self.hop
        self.rows_done += r
        if used < have:
            self.tail = have - used
        else:
            self.tail, self.skip = 0, self.skip + used - have
        return r


def brute_force(n, hop, group, length):
    """(rows, tail, skip) of a stream of `length` samples, straight from the definition."""
    rows = 0
    while (rows * group + group - 1) * hop + n <= length:
        rows += 1
    start = rows * group * hop
    return rows, max(length - start, 0), max(start - length, 0)


def ragged_sizes(seed, total, most=None):
    """Seeded push sizes that sum to `total`: odd ones, 1-sample ones, a few large ones."""
    rng = np.random.default_rng(seed)
    most = most or max(total // 8, 2)
    sizes, left = [], total
    while left > 0:
        kind = rng.integers(0, 4)
        m = 1 if kind == 0 else int(rng.integers(1, 16)) | 1 if kind == 1 else int(rng.integers(1, most + 1))
        m = min(m, left)
        sizes.append(m)
        left -= m
    return sizes


def samples_for(n, hop, rows_out, group):
    return (rows_out * group - 1) * hop + n


def i16_to_float(i16):
    """c(s) = s * 2^-11 as float32: exact over the whole int16 range (what sdrhip_convert_i16_run and oracle.convert_i16 give)."""
    return np.asarray(i16, np.int16).astype(np.float32) * np.float32(2.0 ** -11)


def stream(fmt, nsamples, seed=1620):
    """Interleaved IQ in the pipe's own type: u8, the same as exact floats, or tuner_i16_cases.stream_i16 (full range, forced values)."""
    if fmt == "i16":
        return IC.stream_i16(nsamples, seed=seed)
    u8 = np.random.default_rng(seed).integers(0, 256, 2 * nsamples, dtype=np.uint8)
    if fmt == "cf32":
        return (u8.astype(np.float32) - np.float32(128.0)) * np.float32(1.0 / 128.0)
    return u8


def model_input(fmt, iq):
    """(interleaved samples, spectrum_model format) the numpy model takes for a stream of this type."""
    if fmt == "i16":
        return i16_to_float(iq), M.IQ_CF32
    return iq, (M.IQ_U8 if fmt == "u8" else M.IQ_CF32)


def cut(iq, sizes):
    edges = np.concatenate([[0], np.cumsum(sizes)])
    return [iq[2 * a:2 * b] for a, b in zip(edges[:-1], edges[1:])]


class StateHeader(C.Structure):
    """The head of a saved waterfall Pipe state, as the header documents it."""
    _fields_ = [("magic", C.c_uint32), ("version", C.c_uint32), ("kind", C.c_int32), ("n", C.c_int32), ("input_type", C.c_int32),
                ("group", C.c_int32), ("reduce", C.c_int32), ("unit", C.c_int32), ("hop", C.c_int64), ("floor_db", C.c_double),
                ("pos", C.c_int64), ("rows_done", C.c_int64), ("skip", C.c_int64), ("tail_n", C.c_int64), ("pending", C.c_int64)]


def patch_state(state, **fields):
    h = StateHeader.from_buffer_copy(state[:C.sizeof(StateHeader)])
    for k, v in fields.items():
        setattr(h, k, v)
    return bytes(h) + state[C.sizeof(StateHeader):]


def existing_kind_states(hip):
    """pipe_am_bank_cases.existing_kind_states plus the tenth kind that existed before the waterfall Pipe's: an AM bank Pipe with
    dcBlocker on u8 blocks, after the same three pushes, a flush and a save.  Only calls that the parent tree has."""
    import pipe_am_bank_cases as PC
    import signals as S
    import test_gpu_tuner as T
    states = PC.existing_kind_states(hip)
    tabs = [T.osc_table(1000), np.array([1.0, 0.0], np.float32), T.osc_table(5)]
    p = hip.Pipe.am_bank(hip.AmBank(hip.TunerBank(8, S.taps_decim127(), tabs), dc_block=True), 1000, input_u8=True)
    p.set_adaptive(0)
    u8 = PC.stream("u8", 3 * PC.B)
    for i in range(3):
        p.push(u8[2 * PC.B * i:2 * PC.B * (i + 1)])
    p.flush()
    states["am_bank"] = p.save()
    return states


# sha256 of existing_kind_states(hip)["am_bank"] with `hip` bound to a build of the PARENT commit's tree, printed on an MI355X by a
# throw-away script that imported this function; the other nine are pipe_am_bank_cases.PARENT_STATE_SHA256
PARENT_AM_BANK_STATE_SHA256 = "30466aa5dc1a208909c52ba9f7a16c6a4947f75898e50888b803b895269ef467"      # 1156 bytes
