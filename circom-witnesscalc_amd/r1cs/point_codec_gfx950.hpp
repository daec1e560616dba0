// BN254 points in compressed form (arkworks 0.4 CanonicalSerialize with Compress::Yes, restated from memory:
// include/graph_witness_groth16_compressed.h has the format), and the square roots in Fq and Fq2 that decoding needs.  Host and
// device share this code (FRD); codec.hip runs it one thread per point, the compressed key loader runs it on the host.
//
// A compressed point is x alone, canonical little-endian (G1: 32 B; G2: x.c0 then x.c1, 64 B), with two flags in the top two
// bits of the last byte (free, since q < 2^254): 0x40 the point at infinity (every other bit zero), 0x80 "y is the larger of
// y and -y".  Larger is decided on canonical integers, y > q - y, in Fq2 by c1 first and by c0 when c1 = 0; comparing
// Montgomery limbs would give another answer.
//
// Decoding is strict, stricter than arkworks where noted: both flags, the infinity flag beside any other nonzero bit (arkworks
// ignores x there), a masked coordinate >= q, and an x for which x^3 + b has no root are all refused (CODEC_POINT), and the
// point (0, 0) is written.  A decoded point lies on its curve by construction; subgroup membership is not looked at.
// Encoding does not validate: its input is canonical (or Montgomery) below q and on its curve, or (0, 0).
#pragma once
#include "bn254_points_gfx950.hpp"

namespace cwc_g16 {

constexpr uint32_t CODEC_OK = 0u, CODEC_POINT = 2u;  // GWB_G16V_VALID, GWB_G16V_POINT
constexpr uint32_t G1_COMPRESSED_BYTES = 32, G2_COMPRESSED_BYTES = 64;
constexpr uint32_t CODEC_FLAG_LARGER = 0x80000000u, CODEC_FLAG_INFINITY = 0x40000000u;  // in limb 7 (byte 31: 0x80, 0x40)

// (q + 1) / 4, the exponent of a square root (q = 3 mod 4); 252 bits
#define CWC_QP1D4_LIMBS {0xb61f3f52u, 0x4f082305u, 0x5a1c72a3u, 0x65e05aa4u, 0xa0605617u, 0x6e14116du, 0xb84c680au, 0x0c19139cu}
FRD Fq fq_half_q() { return Fq{{0x6c3e7ea3u, 0x9e10460bu, 0xb438e546u, 0xcbc0b548u, 0x40c0ac2eu, 0xdc2822dbu, 0x7098d014u, 0x18322739u}}; }  // (q - 1) / 2
FRD Fq fq_inv2() { return Fq{{0x4f060572u, 0x87bee7d2u, 0x2f1c6ae5u, 0xd0fd2addu, 0xfcfd4f44u, 0x8f5f7492u, 0x3d9cbfacu, 0x1f37631au}}; }  // R / 2 mod q

// a^((q + 1) / 4), Montgomery in and out: the same uniform square-and-multiply loop as fq_inv, the exponent fixed
FRD Fq fq_pow_qp1d4(const Fq& a) {
    const uint32_t e[8] = CWC_QP1D4_LIMBS;
    Fq acc = fq_one();
    for (int b = 251; b >= 0; --b) {
        acc = fq_sqr(acc);
        if ((e[b >> 5] >> (b & 31)) & 1u) acc = fq_mul(acc, a);
    }
    return acc;
}

// root = a^((q + 1) / 4) (Montgomery, reduced); true iff root^2 == a, that is iff a is a square (0 included, root 0)
FRD bool fq_sqrt(const Fq& a, Fq& root) {
    root = fq_pow_qp1d4(a);
    return cwc::u256_eq(fq_sqr(root), a);
}

// A square root in Fq2 = Fq[u]/(u^2 + 1) from two exponentiations and one inversion, none of them data dependent:
// s = sqrt(a0^2 + a1^2) (the norm of a square is a square), t = (a0 + s) / 2, c = t^((q + 1) / 4).  c^2 is t or -t, since
// t^((q + 1) / 2) = t t^((q - 1) / 2).  With d = a1 / (2 c): c^2 = t gives the root c + d u, c^2 = -t gives d + c u (because
// t (t - s) = -a1^2 / 4 and -1 is no square).  t = 0 would mean a1 = 0 and a0 = -s; the other root -s of the norm is taken then, so
// t = a0 and the two cases are sqrt(a0) and u sqrt(-a0).  c = 0 only for a = 0.  The result is accepted iff its square is a.
FRD bool fq2_sqrt(const Fq2& a, Fq2& root) {
    Fq s;
    const bool norm_ok = fq_sqrt(fq_add(fq_sqr(a.c0), fq_sqr(a.c1)), s);
    const Fq sum = fq_add(a.c0, s);
    const Fq t = fq_mul(cwc::u256_select(cwc::u256_is_zero(sum), fq_sub(a.c0, s), sum), fq_inv2());
    const Fq c = fq_pow_qp1d4(t);
    const Fq d = fq_mul(a.c1, fq_inv(fq_dbl(c)));  // c = 0: d = 0
    const bool plus = cwc::u256_eq(fq_sqr(c), t);
    root = Fq2{cwc::u256_select(plus, c, d), cwc::u256_select(plus, d, c)};
    return cwc::both(norm_ok, Fq2T::eq(fq2_sqr(root), a));
}

// y > q - y for a canonical y below q: y > (q - 1) / 2
FRD bool fq_is_larger(const Fq& y) { return cwc::u256_lt(fq_half_q(), y); }
// the same in Fq2, canonical coefficients: decided by c1, by c0 when c1 = 0
FRD bool fq2_is_larger(const Fq2& y) { return cwc::u256_is_zero(y.c1) ? fq_is_larger(y.c0) : fq_is_larger(y.c1); }

// what the codec needs of a group: the coordinate's words, the sign rule, the root
struct G1Codec {
    using T = G1;
    static constexpr uint32_t WORDS = 1, POINT_BYTES = 64, COMPRESSED_BYTES = G1_COMPRESSED_BYTES;
    static FRD Fq get(const uint8_t* p) { return rd_fq(p); }
    static FRD void put(uint8_t* p, const Fq& v) { wr_fq(p, v); }
    static FRD Fq& top(Fq& x) { return x; }  // the coefficient that carries the flags
    static FRD bool reduced(const Fq& x) { return cwc::u256_lt(x, fq_p()); }
    static FRD Fq to_mont(const Fq& x) { return fq_to_mont(x); }
    static FRD Fq from_mont(const Fq& x) { return fq_from_mont(x); }
    static FRD bool larger(const Fq& y) { return fq_is_larger(y); }
    static FRD bool sqrt(const Fq& a, Fq& r) { return fq_sqrt(a, r); }
    static FRD Fq select(bool c, const Fq& a, const Fq& b) { return cwc::u256_select(c, a, b); }  // c ? a : b
};
struct G2Codec {
    using T = G2;
    static constexpr uint32_t WORDS = 2, POINT_BYTES = 128, COMPRESSED_BYTES = G2_COMPRESSED_BYTES;
    static FRD Fq2 get(const uint8_t* p) { return Fq2{rd_fq(p), rd_fq(p + 32)}; }
    static FRD void put(uint8_t* p, const Fq2& v) {
        wr_fq(p, v.c0);
        wr_fq(p + 32, v.c1);
    }
    static FRD Fq& top(Fq2& x) { return x.c1; }
    static FRD bool reduced(const Fq2& x) { return cwc::both(cwc::u256_lt(x.c0, fq_p()), cwc::u256_lt(x.c1, fq_p())); }
    static FRD Fq2 to_mont(const Fq2& x) { return Fq2{fq_to_mont(x.c0), fq_to_mont(x.c1)}; }
    static FRD Fq2 from_mont(const Fq2& x) { return Fq2{fq_from_mont(x.c0), fq_from_mont(x.c1)}; }
    static FRD bool larger(const Fq2& y) { return fq2_is_larger(y); }
    static FRD bool sqrt(const Fq2& a, Fq2& r) { return fq2_sqrt(a, r); }
    static FRD Fq2 select(bool c, const Fq2& a, const Fq2& b) { return Fq2{cwc::u256_select(c, a.c0, b.c0), cwc::u256_select(c, a.c1, b.c1)}; }
};

// the stored point at `point` (C::POINT_BYTES, canonical or Montgomery; not validated) -> C::COMPRESSED_BYTES at `out`
template <class C>
FRD void point_encode(const uint8_t* point, bool canonical, uint8_t* out) {
    using E = typename C::T::E;
    E x = C::get(point), y = C::get(point + 32 * C::WORDS);
    if (!canonical) {
        x = C::from_mont(x);
        y = C::from_mont(y);
    }
    const bool inf = cwc::both(C::T::is_zero(x), C::T::is_zero(y));
    C::top(x).v[7] |= inf ? CODEC_FLAG_INFINITY : C::larger(y) ? CODEC_FLAG_LARGER : 0u;
    C::put(out, x);
}

// C::COMPRESSED_BYTES at `in` -> the stored point at `point` (canonical or Montgomery) and CODEC_OK, or (0, 0) and CODEC_POINT
template <class C>
FRD uint32_t point_decode(const uint8_t* in, bool canonical, uint8_t* point) {
    using T = typename C::T;
    using E = typename T::E;
    E x = C::get(in);
    const uint32_t flags = C::top(x).v[7] & (CODEC_FLAG_LARGER | CODEC_FLAG_INFINITY);
    C::top(x).v[7] &= ~(CODEC_FLAG_LARGER | CODEC_FLAG_INFINITY);
    bool ok = C::reduced(x);
    const bool inf = flags == CODEC_FLAG_INFINITY;
    if (flags == (CODEC_FLAG_LARGER | CODEC_FLAG_INFINITY)) ok = false;
    if (inf && !T::is_zero(x)) ok = false;
    E xm = T::zero(), ym = T::zero(), yc = T::zero();
    if (ok && !inf) {  // (lanes of refused and infinite points wait here for their wave)
        xm = C::to_mont(x);
        ok = C::sqrt(T::add(T::mul(T::sqr(xm), xm), curve_b<T>()), ym);
        yc = C::from_mont(ym);
        const bool want_larger = flags == CODEC_FLAG_LARGER;
        if (T::is_zero(ym)) {
            if (want_larger) ok = false;  // y = 0 has no larger root (no such point exists: both group orders are odd)
        } else if (C::larger(yc) != want_larger) {
            ym = T::neg(ym);
            yc = T::neg(yc);
        }
    }
    const bool none = cwc::either(!ok, inf);  // limb selects, not a choice between objects: that would put them on the stack
    C::put(point, C::select(none, T::zero(), C::select(canonical, x, xm)));
    C::put(point + 32 * C::WORDS, C::select(none, T::zero(), C::select(canonical, yc, ym)));
    return ok ? CODEC_OK : CODEC_POINT;
}

FRD void g1_encode(const uint8_t* point, bool canonical, uint8_t* out) { point_encode<G1Codec>(point, canonical, out); }
FRD void g2_encode(const uint8_t* point, bool canonical, uint8_t* out) { point_encode<G2Codec>(point, canonical, out); }
FRD uint32_t g1_decode(const uint8_t* in, bool canonical, uint8_t* point) { return point_decode<G1Codec>(in, canonical, point); }
FRD uint32_t g2_decode(const uint8_t* in, bool canonical, uint8_t* point) { return point_decode<G2Codec>(in, canonical, point); }

}  // namespace cwc_g16
