// first_mac.hpp -- the first multiply-add of a lane partial, as ONE instruction.
//
// The reference starts every lane partial at +0 and adds ROUNDED products to it (separate multiply and add: the library is compiled
// with -ffp-contract=off for that reason).  The first of those additions is an addition to +0, and
//
//     +0 + round(a * b)  ==  fma(a, b, +0)          bit for bit, for every a and b:
//
// * fma rounds once, from the exact a * b + 0 = a * b: the same value, the same rounding, the same grid as the multiply's (overflow
//   to Inf and the denormal range included), and adding +0 to a rounded value changes nothing;
// * a product that is -0 (or underflows to -0) gives +0 either way: (+0) + (-0) = +0 in round-to-nearest, and an fma whose exact
//   result is zero from a zero product and a +0 addend is that same sum of zeros;
// * NaN and Inf operands give NaN / Inf either way (x + 0 = x; Inf * 0 = NaN in both forms).
// (LABNOTES uses the same identity for the matrix pipe: D = fma(A, B, +0) = round(A * B).)
//
// A plain `acc = p` would NOT do: it leaves -0 where the reference has +0.  The addend must be the literal +0 -- an fma onto a partial
// that already holds a product rounds once where the reference rounds twice.
//
// SDRHIP_FIRST_MAC_UNFUSED (a build switch for A/B measurements, tools/pass_energy_ab.py): the multiply and the addition as two
// instructions, as the kernels had them before.
#pragma once

namespace sdrhip {

typedef float first_mac_f2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ float first_mac(float a, float b)
{
#ifdef SDRHIP_FIRST_MAC_UNFUSED
    return 0.0f + a * b;
#else
    return __builtin_fmaf(a, b, 0.0f);
#endif
}

__device__ __forceinline__ first_mac_f2 first_mac(first_mac_f2 a, first_mac_f2 b)
{
#ifdef SDRHIP_FIRST_MAC_UNFUSED
    return first_mac_f2{0.0f, 0.0f} + a * b;
#else
    return __builtin_elementwise_fma(a, b, first_mac_f2{0.0f, 0.0f});
#endif
}

// 2-vector of samples by one tap (the systolic decimator: the tap is an SGPR operand)
__device__ __forceinline__ first_mac_f2 first_mac(first_mac_f2 a, float b) { return first_mac(a, first_mac_f2{b, b}); }

}  // namespace sdrhip
