"""The `ref` fixture's provider: the reference's own compiled C (oracle/_ref) where it was built, and everywhere else the
answers it gave, as recorded in tests/golden/ref_answers.json.

oracle/_ref is compiled only where the reference's sources are (oracle/Makefile), so a checkout on its own has no reference
build.  The tests that compare against it ask it through the methods below; each call is keyed by the method, the symbol,
the scalar arguments and the bytes of every input array, and the record keeps, per key, the size and a BLAKE2b digest of
the float32 bit pattern of the answer (plus the end group of the resamplers and the final state of dcBlocker).  Bit
equality with a recorded answer is equality of the digest, so the tests assert exactly what they did against the live build.

    live build present  -> its answers; every one that is also in the record must agree with it (a stale record fails)
    no live build       -> the recorded answers (SDRHIP_REF_REPLAY=1 forces this even where the live build exists)
    SDRHIP_REF_RECORD=PATH (live build required) -> its answers, and every call is written to PATH, merged into what the
                           committed record holds: the way to regenerate tests/golden/ref_answers.json, e.g.
        SDRHIP_REF_RECORD=tests/golden/ref_answers.json python -m pytest tests/test_oracle_vs_ref.py tests/test_dc_blocker.py \
            tests/test_oracle_value_classes.py
    and the same for the GPU tests that ask the reference (tests/test_gpu_dropin.py) on a GPU machine with oracle/_ref.
"""
import contextlib
import ctypes as C
import hashlib
import json
import os

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
RECORD = os.path.join(HERE, "golden", "ref_answers.json")


def bits_digest(a):
    """BLAKE2b-128 of the float32 bit pattern of `a` (what assert_bit_equal compares)."""
    return hashlib.blake2b(np.ascontiguousarray(a, dtype=np.float32).tobytes(), digest_size=16).hexdigest()


NAN_BITS = 0x7FC00000


def canonical_nan(a):
    """`a` as float32 with every NaN replaced by the one pattern 0x7fc00000: sign and payload of a NaN are not part of any comparison
    (tests/value_classes.py), every other bit is."""
    a = np.array(a, dtype=np.float32, copy=True)
    a.view(np.uint32)[np.isnan(a)] = NAN_BITS
    return a


def _f32_bits(v):
    return int(np.array([v], np.float32).view(np.uint32)[0])


def _f32_from_bits(b):
    return np.array([b], np.uint32).view(np.float32)[0]


class RecordedArray:
    """A recorded answer: its element count and the digest of its bits.  conftest.assert_bit_equal compares an array with it."""

    def __init__(self, size, digest, call, canon=False):
        self.size, self.digest, self.call, self.canon = size, digest, call, canon      # canon: the digest was taken after canonical_nan

    def mismatch(self, a):
        """None when `a` has exactly the recorded bits, else what differs."""
        a = np.ascontiguousarray(a, dtype=np.float32).ravel()
        if a.size != self.size:
            return f"{a.size} elements against the reference build's {self.size} ({self.call})"
        if bits_digest(canonical_nan(a) if self.canon else a) != self.digest:
            return f"the bits of the {a.size} elements differ from the reference build's recorded answer ({self.call})"
        return None


def _key(method, *args):
    """Digest of one call: method, scalars and input arrays (dtype, shape, bytes) in order."""
    h = hashlib.sha256(method.encode())
    for a in args:
        if isinstance(a, np.ndarray):
            a = np.ascontiguousarray(a)
            h.update(f"|{a.dtype.str}{a.shape}|".encode())
            h.update(a.tobytes())
        else:
            h.update(f"|{a!r}".encode())
    return h.hexdigest()[:32]


def _prep_args(prep):
    """The fields of an oracle.prepare_coeffs result that Ref.resample passes to the reference."""
    return (int(prep["num_coeffs"]), int(prep["num_groups"]), np.ascontiguousarray(prep["increments"], np.int32),
            np.ascontiguousarray(prep["groups"], np.float32))


def _calls():
    """method -> (key arguments, description) of every call the tests make (one table for live, recording and replay)."""
    return {
        "convert": lambda sym, u8: ((sym, np.ascontiguousarray(u8, np.uint8)), f"{sym} n={np.size(u8)}"),
        "convert_i16": lambda sym, i16: ((sym, np.ascontiguousarray(i16, np.int16)), f"{sym} n={np.size(i16)}"),
        "filt": lambda sym, num, c, x, complex_=False: ((sym, int(num), np.ascontiguousarray(c, np.float32), np.ascontiguousarray(x, np.float32),
                                                         bool(complex_)), f"{sym} num={num} taps={np.size(c)}"),
        "decim": lambda sym, num, factor, c, x, complex_=False: ((sym, int(num), int(factor), np.ascontiguousarray(c, np.float32),
                                                                  np.ascontiguousarray(x, np.float32), bool(complex_)),
                                                                 f"{sym} num={num} factor={factor} taps={np.size(c)}"),
        "resample": lambda sym, buf_size, prep, g0, x, complex_=False: ((sym, int(buf_size)) + _prep_args(prep) + (int(g0), np.ascontiguousarray(x, np.float32),
                                                                        bool(complex_)), f"{sym} num={buf_size} start group {g0}"),
        "resample_legacy": lambda buf_size, interp, decim, fo, c, x: ((int(buf_size), int(interp), int(decim), int(fo), np.ascontiguousarray(c, np.float32),
                                                                       np.ascontiguousarray(x, np.float32)),
                                                                      f"resampleRR num={buf_size} {interp}/{decim} offset {fo}"),
        "scale": lambda sym, factor, x: ((sym, _f32_bits(factor), np.ascontiguousarray(x, np.float32)), f"{sym} factor={factor!r} n={np.size(x)}"),
        "convert_tx": lambda x: ((np.ascontiguousarray(x, np.float32),), f"convertBladeRFTransmit n={np.size(x)}"),
        "dc_blocker": lambda x, ls=0.0, lo=0.0: ((np.ascontiguousarray(x, np.float32), _f32_bits(ls), _f32_bits(lo)), f"dcBlocker n={np.size(x)}"),
    }


def _split(method, answer):
    """(array, extras) of a live answer; extras are the scalars the record keeps as they are."""
    if method == "resample":
        return answer[0], {"group": int(answer[1])}
    if method == "dc_blocker":
        return answer[0], {"final": [_f32_bits(answer[1]), _f32_bits(answer[2])]}
    return answer, {}


def _join(method, arr, entry):
    if method == "resample":
        return arr, int(entry["group"])
    if method == "dc_blocker":
        return arr, _f32_from_bits(entry["final"][0]), _f32_from_bits(entry["final"][1])
    return arr


class _Live:
    """The live build, with the one call the oracle's Ref wrapper has no method for."""

    def __init__(self, ref):
        self.ref = ref

    def convert_i16(self, sym, i16):
        i16 = np.ascontiguousarray(i16, np.int16)
        out = np.empty(i16.size + 8, np.float32)
        buf = np.zeros(i16.size + 16, np.int16)          # the SSE / AVX variants read past the input's end
        buf[:i16.size] = i16
        getattr(self.ref.lib, sym)(C.c_int(i16.size), buf.ctypes.data_as(C.POINTER(C.c_int16)), out.ctypes.data_as(C.POINTER(C.c_float)))
        return out[:i16.size].copy()

    def convert_tx(self, x):
        """int16 answers: as float32 they are exact, so the record's digest of float32 bits serves."""
        x = np.ascontiguousarray(x, np.float32)
        out = np.empty(x.size, np.int16)
        self.ref.lib.convertBladeRFTransmit(C.c_int(x.size), x.ctypes.data_as(C.POINTER(C.c_float)), out.ctypes.data_as(C.POINTER(C.c_int16)))
        return out

    def __getattr__(self, name):
        return getattr(self.ref, name)


class RefAnswers:
    """What the tests call `ref`: live (checked against the record), recording, or replaying the record."""

    def __init__(self, live=None, record_to=None):
        self.live = _Live(live) if live is not None else None
        self.record_to = record_to
        self.table = json.load(open(RECORD)) if os.path.exists(RECORD) else {}
        self.last_key = list(self.table)[-1] if self.table else None
        if record_to and os.path.exists(record_to):
            self.table.update(json.load(open(record_to)))
        self.recorded = {}
        self.canon = False
        for method, describe in _calls().items():
            setattr(self, method, self._method(method, describe))

    def _method(self, method, describe):
        def call(*args, **kw):
            key_args, what = describe(*args, **kw)
            key = _key(method, *key_args)
            entry = self.table.get(key)
            if self.live is None:
                if entry is None:
                    pytest.fail(f"no recorded answer of the reference build for {method} {what}: regenerate tests/golden/ref_answers.json "
                                "where oracle/_ref exists (tests/ref_answers.py)")
                assert bool(entry.get("canon", False)) == self.canon, f"{method} {what}: recorded with canon = {entry.get('canon', False)}"
                return _join(method, RecordedArray(entry["n"], entry["b2"], f"{method} {what}", self.canon), entry)
            answer = getattr(self.live, method)(*args, **kw)
            arr, extras = _split(method, answer)
            if self.canon and "final" in extras:             # a NaN final state is recorded as the one canonical pattern too
                extras["final"] = [NAN_BITS if (b & 0x7FFFFFFF) > 0x7F800000 else b for b in extras["final"]]
            new = {"n": int(np.size(arr)), "b2": bits_digest(canonical_nan(arr) if self.canon else arr), "call": f"{method} {what}", **extras}
            if self.canon:
                new["canon"] = True
            if entry is not None and not self.record_to:
                assert {k: entry.get(k) for k in new if k != "call"} == {k: v for k, v in new.items() if k != "call"}, \
                    f"tests/golden/ref_answers.json disagrees with the reference build on {method} {what}: regenerate it"
            if self.record_to:
                self.recorded[key] = new
            return answer
        return call

    @contextlib.contextmanager
    def canonical(self):
        """Calls made inside compare and record their answers with NaNs made canonical (canonical_nan); their entries carry
        "canon": true, and RecordedArray.mismatch then treats the array it is given the same way."""
        prev, self.canon = self.canon, True
        try:
            yield self
        finally:
            self.canon = prev

    def close(self):
        if self.record_to and self.recorded:
            self.table.update(self.recorded)
            keys = sorted(self.table)
            if self.last_key in self.table:              # the record's last line stays last (it alone has no comma): regenerating adds lines only
                keys.remove(self.last_key)
                keys.append(self.last_key)
            with open(self.record_to, "w") as f:         # one answer per line
                f.write("{\n" + ",\n".join(f"{json.dumps(k)}: {json.dumps(self.table[k], sort_keys=True)}" for k in keys) + "\n}\n")


def open_ref():
    from oracle.oracle import Ref, build, have_ref
    record_to = os.environ.get("SDRHIP_REF_RECORD") or None
    if os.environ.get("SDRHIP_REF_REPLAY") == "1" and not record_to:
        return RefAnswers()
    if not have_ref():
        build()                     # oracle/Makefile compiles oracle/_ref where the reference's sources are, and nothing else
    if have_ref():
        return RefAnswers(Ref(), record_to)
    if record_to:
        pytest.fail("SDRHIP_REF_RECORD needs the reference build (oracle/_ref)")
    return RefAnswers()
