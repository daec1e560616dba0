// BN254 points as the files and the C ABI store them, decoded and encoded in one place, for the loaders (zkey.cc, ptau.cc), the
// key setups, the prover, the verifier and the G2 subgroup check.  Host and device share this code (FRD).
//
// The stored form: affine, every coordinate 8 x u32 little-endian limbs (32 bytes) and below q, in Montgomery form (R = 2^256,
// the files) or canonical (the C ABI's points); a G1 point is x, y, a G2 point x.c0, x.c1, y.c0, y.c1; all-zero bytes are the
// point at infinity; every other point lies on its curve, G1: y^2 = x^3 + 3, G2 (the twist): y^2 = x^3 + 3 / (9 + u).
// Subgroup membership is not part of the form (g2_subgroup_gfx950.hpp).  In registers a point is Affine<T> or Xyzz<T> of
// fq_gfx950.hpp, Montgomery form.
#pragma once
#include <string.h>

#include "fq_gfx950.hpp"

namespace cwc_g16 {

#include "fq12_consts_gfx950.inc"  // twist_b(); the rest of the generated constants are the pairing tower's (fq12_gfx950.hpp)

using G1 = FqT;
using G2 = Fq2T;
using A1 = Affine<G1>;
using A2 = Affine<G2>;
using P1 = Xyzz<G1>;
using P2 = Xyzz<G2>;

// what is wrong with a stored point, in the order the loaders look (SUBGROUP: the opt-in G2 check alone)
enum class PointFault : uint32_t { COORDINATE = 0, CURVE = 1, SUBGROUP = 2, NONE = 3 };

// 32 stored bytes <-> the limbs.  Device addresses are aligned as Fq is; host bytes may lie anywhere in a mapped file.
FRD Fq rd_fq(const uint8_t* p) {
#if defined(__HIP_DEVICE_COMPILE__)
    return *reinterpret_cast<const Fq*>(p);
#else
    Fq v;
    memcpy(v.v, p, 32);
    return v;
#endif
}
FRD void wr_fq(uint8_t* p, const Fq& v) {
#if defined(__HIP_DEVICE_COMPILE__)
    *reinterpret_cast<Fq*>(p) = v;
#else
    memcpy(p, v.v, 32);
#endif
}

// the curve's constant b, Montgomery form
template <class T>
FRD typename T::E curve_b();
template <>
FRD Fq curve_b<G1>() { return Fq{{0x50ad28d7u, 0x7a17caa9u, 0xe15521b9u, 0x1f6ac17au, 0x696bd284u, 0x334bea4eu, 0xce179d8eu, 0x2a1f6744u}}; }  // 3 R mod q
template <>
FRD Fq2 curve_b<G2>() { return twist_b(); }

// the coordinates at `in` (Montgomery form out); false when one of them is not below q
template <class T>
FRD bool get_coords(const uint8_t* in, bool canonical, typename T::E& x, typename T::E& y);
template <>
FRD bool get_coords<G1>(const uint8_t* in, bool canonical, Fq& x, Fq& y) {
    const Fq a = rd_fq(in), b = rd_fq(in + 32);
    const bool ok = cwc::both(cwc::u256_lt(a, fq_p()), cwc::u256_lt(b, fq_p()));
    x = canonical ? fq_to_mont(a) : a;
    y = canonical ? fq_to_mont(b) : b;
    return ok;
}
template <>
FRD bool get_coords<G2>(const uint8_t* in, bool canonical, Fq2& x, Fq2& y) {
    const Fq a = rd_fq(in), b = rd_fq(in + 32), d = rd_fq(in + 64), e = rd_fq(in + 96);
    const bool ok = cwc::both(cwc::both(cwc::u256_lt(a, fq_p()), cwc::u256_lt(b, fq_p())), cwc::both(cwc::u256_lt(d, fq_p()), cwc::u256_lt(e, fq_p())));
    x = Fq2{canonical ? fq_to_mont(a) : a, canonical ? fq_to_mont(b) : b};
    y = Fq2{canonical ? fq_to_mont(d) : d, canonical ? fq_to_mont(e) : e};
    return ok;
}

// Montgomery coordinates -> the stored bytes at `out`; (0, 0) writes the point at infinity
template <class T>
FRD void put_coords(uint8_t* out, const typename T::E& x, const typename T::E& y, bool canonical);
template <>
FRD void put_coords<G1>(uint8_t* out, const Fq& x, const Fq& y, bool canonical) {
    wr_fq(out, canonical ? fq_from_mont(x) : x);
    wr_fq(out + 32, canonical ? fq_from_mont(y) : y);
}
template <>
FRD void put_coords<G2>(uint8_t* out, const Fq2& x, const Fq2& y, bool canonical) {
    wr_fq(out, canonical ? fq_from_mont(x.c0) : x.c0);
    wr_fq(out + 32, canonical ? fq_from_mont(x.c1) : x.c1);
    wr_fq(out + 64, canonical ? fq_from_mont(y.c0) : y.c0);
    wr_fq(out + 96, canonical ? fq_from_mont(y.c1) : y.c1);
}

// ZZ = ZZZ = 1, or the point at infinity for (0, 0).  Where the point is known not to be infinity, the plain initialiser
// {x, y, 1, 1} stands instead (g2_mul_x, table_bases_kernel): the test would be dead work there.
template <class T>
FRD Xyzz<T> from_affine(const Affine<T>& a) {
    return affine_is_inf(a) ? xyzz_inf<T>() : Xyzz<T>{a.x, a.y, T::one(), T::one()};
}

// the stored point at `in` into p, and what is wrong with it: a coordinate >= q, else infinity passes, else the curve equation
template <class T>
FRD PointFault get_point(const uint8_t* in, bool canonical, Affine<T>& p) {
    if (!get_coords<T>(in, canonical, p.x, p.y)) return PointFault::COORDINATE;
    if (affine_is_inf(p)) return PointFault::NONE;
    return on_curve<T>(p, curve_b<T>()) ? PointFault::NONE : PointFault::CURVE;
}
template <class T>
FRD PointFault point_fault(const uint8_t* in, bool canonical) {
    Affine<T> p;
    return get_point<T>(in, canonical, p);
}

FRD A1 g1_generator() { return A1{fq_one(), fq_add(fq_one(), fq_one())}; }  // (1, 2)
FRD A2 g2_generator() {
    const Fq c[4] = {{{0xd992f6edu, 0x46debd5cu, 0xf75edaddu, 0x674322d4u, 0x5e5c4479u, 0x426a0066u, 0x121f1e76u, 0x1800deefu}},
                     {{0xaef312c2u, 0x97e485b7u, 0x35a9e712u, 0xf1aa4933u, 0x31fb5d25u, 0x7260bfb7u, 0x920d483au, 0x198e9393u}},
                     {{0x66fa7daau, 0x4ce6cc01u, 0x0c43d37bu, 0xe3d1e769u, 0x8dcb408fu, 0x4aab7180u, 0xdb8c6debu, 0x12c85ea5u}},
                     {{0xd122975bu, 0x55acdadcu, 0x70b38ef3u, 0xbc4b3133u, 0x690c3395u, 0xec9e99adu, 0x585ff075u, 0x090689d0u}}};
    return A2{Fq2{fq_to_mont(c[0]), fq_to_mont(c[1])}, Fq2{fq_to_mont(c[2]), fq_to_mont(c[3])}};
}

}  // namespace cwc_g16
