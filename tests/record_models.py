"""The reference's Filter / Decimator / Resampler records with both closures bound to the device, in Python: what haskell/SDR/GPU.hs
builds (fastDecimatorCGpu, filterRecord, fastResamplerRGpu), on top of the restated Pipes of oracle/pipes_model.py.  A Pipe run
with one of these models drives sdrhip_{filter,decimator,resampler}_{one,cross} (abi_records.cpp) block by block exactly as the
reference's unchanged firFilter / firDecimator / firResampler would; the same Pipe with the plain model is the expected answer.

Every closure hands the C call the host arrays the Pipe handed it -- the whole `buf` with its full length, never a trimmed copy --
and an output array between guard words (the canary of tests/gpu_util.py, on a host array), which it checks after the call."""
import ctypes as C

import numpy as np

from gpu_util import CANARY, GUARD
from oracle import pipes_model as PM

_f32p = C.POINTER(C.c_float)


def _fp(a):
    return a.ctypes.data_as(_f32p)


class GuardedOut:
    """n floats between two bands of GUARD canary words; the payload starts as canaries too, so `untouched` can tell."""

    def __init__(self, n):
        self.n = int(n)
        self.whole = np.full(self.n + 2 * GUARD, CANARY, np.uint32)
        self.out = self.whole[GUARD:GUARD + self.n].view(np.float32)

    def check(self, what):
        lo, hi = self.whole[:GUARD], self.whole[GUARD + self.n:]
        bad_lo, bad_hi = int((lo != CANARY).sum()), int((hi != CANARY).sum())
        assert bad_lo == 0 and bad_hi == 0, (f"{what}: the call wrote outside its output of {self.n} floats: {bad_lo} guard words before it, "
                                             f"{bad_hi} behind it were overwritten")

    def untouched(self):
        return bool((self.whole == CANARY).all())


def _checked(L, rc, what):
    """A negative status raises with the library's own message, as GPU.hs's `check` does."""
    if rc < 0:
        raise L.SdrHipError(f"{what} failed ({rc}): {L.lib.sdrhip_last_error().decode()}")
    return rc


class DeviceFilterModel(PM.FilterModel):
    """Filter { filterOne, filterCross } / Decimator { decimateOne, decimateCross } on the device (GPU.hs: filterRecord,
    fastDecimatorCGpu).  factor == 1 makes a hip.Filter, anything else a hip.Decimator, as the fast* constructors do."""

    def __init__(self, oracle, coeffs, order=PM.ORDER_AVX, complex_=False, sym=False, factor=1, desc=None):
        super().__init__(oracle, coeffs, order, complex_, sym, factor)
        import sdr_amd.lib as L
        self.L = L
        if desc is not None:
            self.desc = desc                    # shared with another record (descriptors are immutable after create)
        elif factor == 1:
            self.desc = L.Filter(coeffs, order, complex_=complex_, sym=sym)
        else:
            self.desc = L.Decimator(factor, coeffs, order, complex_=complex_, sym=sym)
        self.name = "sdrhip_filter" if isinstance(self.desc, L.Filter) else "sdrhip_decimator"
        assert self.desc.num_coeffs == self.num_coeffs, (self.desc.num_coeffs, self.num_coeffs)

    def one(self, count, buf):
        g = GuardedOut(count * self.width)
        f = getattr(self.L.lib, self.name + "_one")
        _checked(self.L, f(self.desc.h, count, _fp(buf), _fp(g.out)), self.name + "_one")
        g.check(self.name + "_one")
        return g.out

    def cross(self, count, last, nxt):
        g = GuardedOut(count * self.width)
        f = getattr(self.L.lib, self.name + "_cross")
        _checked(self.L, f(self.desc.h, count, _fp(last), last.size // self.width, _fp(nxt), nxt.size // self.width, _fp(g.out)),
                 self.name + "_cross")
        g.check(self.name + "_cross")
        return g.out


class DeviceResamplerModel(PM.ResamplerModel):
    """Resampler { resampleOne, resampleCross } on the device, carrying (group, offset) as mkResampler does (Filter.hs:408-425) with
    the formulas of GPU.hs's fastResamplerRGpu."""

    def __init__(self, oracle, interpolation, decimation, coeffs, order=PM.ORDER_AVX, complex_=False, desc=None):
        super().__init__(oracle, interpolation, decimation, coeffs, order, complex_)
        import sdr_amd.lib as L
        self.L = L
        self.desc = desc if desc is not None else L.Resampler(interpolation, decimation, coeffs, order, complex_=complex_)
        assert self.desc.num_coeffs == self.num_coeffs, (self.desc.num_coeffs, self.num_coeffs)

    def one(self, dat, count, buf):
        group = dat[0]
        g = GuardedOut(count * self.width)
        group2 = _checked(self.L, self.L.lib.sdrhip_resampler_one(self.desc.h, group, count, _fp(buf), buf.size // self.width, _fp(g.out)),
                          "sdrhip_resampler_one")
        g.check("sdrhip_resampler_one")
        offset = self.I - 1 - ((self.I + group2 * self.D - 1) % self.I)                 # offsetOf, GPU.hs
        return g.out, (group2, offset), offset

    def cross(self, dat, count, last, nxt):
        group, offset = dat
        g = GuardedOut(count * self.width)
        w = self.width
        offset2 = _checked(self.L, self.L.lib.sdrhip_resampler_cross(self.desc.h, offset, count, _fp(last), last.size // w, _fp(nxt),
                                                                    nxt.size // w, _fp(g.out)), "sdrhip_resampler_cross")
        g.check("sdrhip_resampler_cross")
        return g.out, ((group + count) % self.I, offset2), offset2
