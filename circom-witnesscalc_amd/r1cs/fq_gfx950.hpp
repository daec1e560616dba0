// BN254 base field Fq (q = 21888242871839275222246405745257275088696311157297823662689037894645226208583), its quadratic
// extension Fq2 = Fq[u]/(u^2 + 1), and the G1 / G2 group law, for the Groth16 prover (msm.hip) and the zkey loader's
// curve checks (zkey.cc, host).  8 x u32 limbs, Montgomery form with R = 2^256 (snarkjs's "LEM" coordinates as stored).
//
// The limb helpers are csrc/fr_gfx950.hpp's (included read-only).  Where Fr's code relies on r < 2^254 the same holds for
// q < 2^254: a + b of two reduced values has no carry out of 2^256, and the Montgomery product's quotient stays below 2q.
// The device product is generated (tools/codegen/gen_fq_mul.py, fr_mul's instruction sequence with q's limbs).
#pragma once
#include "../csrc/fr_gfx950.hpp"

namespace cwc_g16 {

using Fq = cwc::Fr;  // the same 8-limb integer; only the modulus differs

#define CWC_Q0 0xd87cfd47u
#define CWC_Q1 0x3c208c16u
#define CWC_Q2 0x6871ca8du
#define CWC_Q3 0x97816a91u
#define CWC_Q4 0x8181585du
#define CWC_Q5 0xb85045b6u
#define CWC_Q6 0xe131a029u
#define CWC_Q7 0x30644e72u
#define CWC_QINV32 0xe4866389u  // -q^-1 mod 2^32

FRD Fq fq_p() { return Fq{{CWC_Q0, CWC_Q1, CWC_Q2, CWC_Q3, CWC_Q4, CWC_Q5, CWC_Q6, CWC_Q7}}; }
FRD Fq fq_one() { return Fq{{0xc58f0d9du, 0xd35d438du, 0xf5c70b3du, 0x0a78eb28u, 0x7879462cu, 0x666ea36fu, 0x9a07df2fu, 0x0e0a77c1u}}; }  // R mod q
FRD Fq fq_r2() { return Fq{{0x538afa89u, 0xf32cfc5bu, 0xd44501fbu, 0xb5e71911u, 0x0a417ff6u, 0x47ab1effu, 0xcab8351fu, 0x06d89f71u}}; }  // R^2 mod q
FRD Fq fq_zero() { return Fq{{0, 0, 0, 0, 0, 0, 0, 0}}; }

FRD Fq fq_add(const Fq& a, const Fq& b) {
    Fq s, t;
    cwc::u256_add(s, a, b);  // < 2q < 2^255
    const uint32_t br = cwc::u256_sub(t, s, fq_p());
    return cwc::u256_select(br != 0, s, t);
}
FRD Fq fq_sub(const Fq& a, const Fq& b) {
    Fq d, t;
    const uint32_t br = cwc::u256_sub(d, a, b);
    cwc::u256_add(t, d, fq_p());
    return cwc::u256_select(br != 0, t, d);
}
FRD Fq fq_dbl(const Fq& a) { return fq_add(a, a); }
FRD Fq fq_neg(const Fq& a) {
    Fq t;
    cwc::u256_sub(t, fq_p(), a);
    return cwc::u256_select(cwc::u256_is_zero(a), a, t);
}

// Montgomery product a b / 2^256 mod q; b < q, a any value below 2^256 (as fr_mul)
FRD Fq fq_mul(const Fq& a, const Fq& b) {
#if defined(__HIP_DEVICE_COMPILE__)
#include "fq_mul_gfx950.inc"
#else
    const uint32_t p[8] = {CWC_Q0, CWC_Q1, CWC_Q2, CWC_Q3, CWC_Q4, CWC_Q5, CWC_Q6, CWC_Q7};
    uint32_t t[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (int i = 0; i < 8; ++i) {
        uint64_t c = 0;
        for (int j = 0; j < 8; ++j) {
            c += (uint64_t)a.v[i] * b.v[j] + t[j];
            t[j] = (uint32_t)c;
            c >>= 32;
        }
        t[8] = (uint32_t)c;
        const uint32_t m = t[0] * CWC_QINV32;
        c = ((uint64_t)m * p[0] + t[0]) >> 32;
        for (int j = 1; j < 8; ++j) {
            c += (uint64_t)m * p[j] + t[j];
            t[j - 1] = (uint32_t)c;
            c >>= 32;
        }
        c += t[8];
        t[7] = (uint32_t)c;
    }
    Fq r, s;
    for (int i = 0; i < 8; ++i) r.v[i] = t[i];
    const uint32_t br = cwc::u256_sub(s, r, fq_p());
    return cwc::u256_select(br != 0, r, s);
#endif
}
FRD Fq fq_sqr(const Fq& a) { return fq_mul(a, a); }
FRD Fq fq_to_mont(const Fq& x) { return fq_mul(x, fq_r2()); }
FRD Fq fq_from_mont(const Fq& x) { return fq_mul(x, Fq{{1, 0, 0, 0, 0, 0, 0, 0}}); }

// a^(q-2) (Fermat; a few per proof), Montgomery in and out; 0 -> 0
FRD Fq fq_inv(const Fq& a) {
    const uint32_t e[8] = {CWC_Q0 - 2u, CWC_Q1, CWC_Q2, CWC_Q3, CWC_Q4, CWC_Q5, CWC_Q6, CWC_Q7};  // q0 > 2: no borrow
    Fq acc = fq_one();
    for (int b = 253; b >= 0; --b) {  // q < 2^254
        acc = fq_sqr(acc);
        if ((e[b >> 5] >> (b & 31)) & 1u) acc = fq_mul(acc, a);
    }
    return acc;
}

// ---- Fq2 = Fq[u]/(u^2 + 1) -------------------------------------------------------------------------------------------------
struct Fq2 {
    Fq c0, c1;
};

FRD Fq2 fq2_add(const Fq2& a, const Fq2& b) { return Fq2{fq_add(a.c0, b.c0), fq_add(a.c1, b.c1)}; }
FRD Fq2 fq2_sub(const Fq2& a, const Fq2& b) { return Fq2{fq_sub(a.c0, b.c0), fq_sub(a.c1, b.c1)}; }
FRD Fq2 fq2_dbl(const Fq2& a) { return Fq2{fq_dbl(a.c0), fq_dbl(a.c1)}; }
FRD Fq2 fq2_neg(const Fq2& a) { return Fq2{fq_neg(a.c0), fq_neg(a.c1)}; }
// Karatsuba: (a0 + a1 u)(b0 + b1 u) = a0 b0 - a1 b1 + ((a0 + a1)(b0 + b1) - a0 b0 - a1 b1) u; three products
FRD Fq2 fq2_mul(const Fq2& a, const Fq2& b) {
    const Fq t0 = fq_mul(a.c0, b.c0), t1 = fq_mul(a.c1, b.c1);
    const Fq t2 = fq_mul(fq_add(a.c0, a.c1), fq_add(b.c0, b.c1));
    return Fq2{fq_sub(t0, t1), fq_sub(fq_sub(t2, t0), t1)};
}
// (a0 + a1 u)^2 = (a0 + a1)(a0 - a1) + 2 a0 a1 u; two products
FRD Fq2 fq2_sqr(const Fq2& a) {
    const Fq t = fq_mul(a.c0, a.c1);
    return Fq2{fq_mul(fq_add(a.c0, a.c1), fq_sub(a.c0, a.c1)), fq_dbl(t)};
}
// 1 / (a0 + a1 u) = (a0 - a1 u) / (a0^2 + a1^2)
FRD Fq2 fq2_inv(const Fq2& a) {
    const Fq n = fq_inv(fq_add(fq_sqr(a.c0), fq_sqr(a.c1)));
    return Fq2{fq_mul(a.c0, n), fq_neg(fq_mul(a.c1, n))};
}

// ---- the group law over either coordinate field ----------------------------------------------------------------------------
// Field traits: E (element), add, sub, dbl, neg, mul, sqr, inv, zero, is_zero, eq.
struct FqT {
    using E = Fq;
    static FRD E add(const E& a, const E& b) { return fq_add(a, b); }
    static FRD E sub(const E& a, const E& b) { return fq_sub(a, b); }
    static FRD E dbl(const E& a) { return fq_dbl(a); }
    static FRD E neg(const E& a) { return fq_neg(a); }
    static FRD E mul(const E& a, const E& b) { return fq_mul(a, b); }
    static FRD E sqr(const E& a) { return fq_sqr(a); }
    static FRD E inv(const E& a) { return fq_inv(a); }
    static FRD E zero() { return fq_zero(); }
    static FRD E one() { return fq_one(); }
    static FRD bool is_zero(const E& a) { return cwc::u256_is_zero(a); }
    static FRD bool eq(const E& a, const E& b) { return cwc::u256_eq(a, b); }
};
struct Fq2T {
    using E = Fq2;
    static FRD E add(const E& a, const E& b) { return fq2_add(a, b); }
    static FRD E sub(const E& a, const E& b) { return fq2_sub(a, b); }
    static FRD E dbl(const E& a) { return fq2_dbl(a); }
    static FRD E neg(const E& a) { return fq2_neg(a); }
    static FRD E mul(const E& a, const E& b) { return fq2_mul(a, b); }
    static FRD E sqr(const E& a) { return fq2_sqr(a); }
    static FRD E inv(const E& a) { return fq2_inv(a); }
    static FRD E zero() { return Fq2{fq_zero(), fq_zero()}; }
    static FRD E one() { return Fq2{fq_one(), fq_zero()}; }
    static FRD bool is_zero(const E& a) { return cwc::both(cwc::u256_is_zero(a.c0), cwc::u256_is_zero(a.c1)); }
    static FRD bool eq(const E& a, const E& b) { return cwc::both(cwc::u256_eq(a.c0, b.c0), cwc::u256_eq(a.c1, b.c1)); }
};

// An affine point as the zkey stores it; (0, 0) is the point at infinity (it is on neither curve).
template <class T>
struct Affine {
    typename T::E x, y;
};
// XYZZ coordinates (x = X / ZZ, y = Y / ZZZ, ZZ^3 = ZZZ^2); ZZ = 0 is the point at infinity, so all-zero bytes are too.
template <class T>
struct Xyzz {
    typename T::E X, Y, ZZ, ZZZ;
};

template <class T>
FRD Xyzz<T> xyzz_inf() {
    return Xyzz<T>{T::zero(), T::zero(), T::zero(), T::zero()};
}
template <class T>
FRD bool xyzz_is_inf(const Xyzz<T>& p) { return T::is_zero(p.ZZ); }
template <class T>
FRD bool affine_is_inf(const Affine<T>& p) { return cwc::both(T::is_zero(p.x), T::is_zero(p.y)); }
template <class T>
FRD Xyzz<T> xyzz_neg(const Xyzz<T>& p) { return Xyzz<T>{p.X, T::neg(p.Y), p.ZZ, p.ZZZ}; }

// dbl-2008-s-1 (a = 0): U = 2Y, V = U^2, W = U V, S = X V, M = 3 X^2, X3 = M^2 - 2S, Y3 = M (S - X3) - W Y
template <class T>
FRD Xyzz<T> xyzz_dbl(const Xyzz<T>& p) {
    if (xyzz_is_inf(p)) return p;
    using E = typename T::E;
    const E U = T::dbl(p.Y), V = T::sqr(U), W = T::mul(U, V), S = T::mul(p.X, V);
    const E X2 = T::sqr(p.X), M = T::add(T::dbl(X2), X2);
    const E X3 = T::sub(T::sqr(M), T::dbl(S));
    const E Y3 = T::sub(T::mul(M, T::sub(S, X3)), T::mul(W, p.Y));
    return Xyzz<T>{X3, Y3, T::mul(V, p.ZZ), T::mul(W, p.ZZZ)};
}

// p + (x, y), madd-2008-s; (x, y) not the point at infinity.  P == Q doubles, P == -Q gives infinity.
template <class T>
FRD Xyzz<T> xyzz_add_affine(const Xyzz<T>& p, const Affine<T>& q) {
    using E = typename T::E;
    if (xyzz_is_inf(p)) return Xyzz<T>{q.x, q.y, T::one(), T::one()};
    const E P = T::sub(T::mul(q.x, p.ZZ), p.X), R = T::sub(T::mul(q.y, p.ZZZ), p.Y);
    if (T::is_zero(P)) {
        if (T::is_zero(R)) return xyzz_dbl(Xyzz<T>{q.x, q.y, T::one(), T::one()});
        return xyzz_inf<T>();
    }
    const E PP = T::sqr(P), PPP = T::mul(P, PP), Q = T::mul(p.X, PP);
    const E X3 = T::sub(T::sub(T::sqr(R), PPP), T::dbl(Q));
    const E Y3 = T::sub(T::mul(R, T::sub(Q, X3)), T::mul(p.Y, PPP));
    return Xyzz<T>{X3, Y3, T::mul(p.ZZ, PP), T::mul(p.ZZZ, PPP)};
}

// p + q, add-2008-s, every special case
template <class T>
FRD Xyzz<T> xyzz_add(const Xyzz<T>& p, const Xyzz<T>& q) {
    using E = typename T::E;
    if (xyzz_is_inf(p)) return q;
    if (xyzz_is_inf(q)) return p;
    const E U1 = T::mul(p.X, q.ZZ), S1 = T::mul(p.Y, q.ZZZ);
    const E P = T::sub(T::mul(q.X, p.ZZ), U1), R = T::sub(T::mul(q.Y, p.ZZZ), S1);
    if (T::is_zero(P)) {
        if (T::is_zero(R)) return xyzz_dbl(p);
        return xyzz_inf<T>();
    }
    const E PP = T::sqr(P), PPP = T::mul(P, PP), Q = T::mul(U1, PP);
    const E X3 = T::sub(T::sub(T::sqr(R), PPP), T::dbl(Q));
    const E Y3 = T::sub(T::mul(R, T::sub(Q, X3)), T::mul(S1, PPP));
    return Xyzz<T>{X3, Y3, T::mul(T::mul(p.ZZ, q.ZZ), PP), T::mul(T::mul(p.ZZZ, q.ZZZ), PPP)};
}

// affine form ((0, 0) for infinity)
template <class T>
FRD Affine<T> xyzz_to_affine(const Xyzz<T>& p) {
    if (xyzz_is_inf(p)) return Affine<T>{T::zero(), T::zero()};
    return Affine<T>{T::mul(p.X, T::inv(p.ZZ)), T::mul(p.Y, T::inv(p.ZZZ))};
}

// k p for a canonical 256-bit k (double-and-add from the top bit)
template <class T>
FRD Xyzz<T> xyzz_mul(const Xyzz<T>& p, const cwc::Fr& k) {
    Xyzz<T> acc = xyzz_inf<T>();
    cwc::Fr kk = k;  // words move up into kk.v[7] (constant indices: no stack copy of k on the device)
    for (int w = 0; w < 8; ++w) {
        const uint32_t word = kk.v[7];
        for (int b = 31; b >= 0; --b) {
            acc = xyzz_dbl(acc);
            if ((word >> b) & 1u) acc = xyzz_add(acc, p);
        }
#pragma unroll
        for (int i = 7; i > 0; --i) kk.v[i] = kk.v[i - 1];
    }
    return acc;
}

// k p for a canonical k: double and add from the top nonzero word of k (inside it the doublings of infinity return at once)
template <class T>
FRD Xyzz<T> xyzz_mul_short(const Xyzz<T>& p, const cwc::Fr& k) {
    Xyzz<T> acc = xyzz_inf<T>();
    cwc::Fr kk = k;  // words move up into kk.v[7] (constant indices: no stack copy of k)
    for (int w = 0; w < 8; ++w) {
        const uint32_t word = kk.v[7];
        if (word != 0 || !xyzz_is_inf(acc)) {
            for (int b = 31; b >= 0; --b) {
                acc = xyzz_dbl(acc);
                if ((word >> b) & 1u) acc = xyzz_add(acc, p);
            }
        }
#pragma unroll
        for (int i = 7; i > 0; --i) kk.v[i] = kk.v[i - 1];
    }
    return acc;
}

// y^2 == x^3 + b (Montgomery coordinates; b in Montgomery form)
template <class T>
FRD bool on_curve(const Affine<T>& p, const typename T::E& b) {
    return T::eq(T::sqr(p.y), T::add(T::mul(T::sqr(p.x), p.x), b));
}

}  // namespace cwc_g16
