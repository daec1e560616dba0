// The BN254 pairing tower and the optimal ate pairing's building blocks, for the Groth16 verifier (verify.hip; the key
// loader's twist check uses the host build).  Definition in include/graph_witness_groth16_verify.h.
//
//   Fq2 = Fq[u]/(u^2 + 1)  (fq_gfx950.hpp),  xi = 9 + u
//   Fq6 = Fq2[v]/(v^3 - xi) = b0 + b1 v + b2 v^2,  Fq12 = Fq6[w]/(w^2 - v) = c0 + c1 w   (so w^6 = xi)
//
// Montgomery form throughout (R = 2^256).  Over Fq2 an Fq12 element is sum_{i<6} g_i w^i with g_0 = c0.b0, g_1 = c1.b0,
// g_2 = c0.b1, g_3 = c1.b1, g_4 = c0.b2, g_5 = c1.b2; the Frobenius maps act as (g w^i)^(q^k) = g^(q^k) gamma_k_i w^i, the
// constants gamma_k_i = xi^(i (q^k - 1) / 6) and the twist constant b' = 3 / xi coming from tools/codegen/gen_fq12_consts.py.
//
// G2 is the D-type twist y^2 = x^3 + b' (untwisted: (x, y) -> (x w^2, y w^3)).  The Miller loop keeps T in homogeneous
// projective coordinates (x = X / Z, y = Y / Z); each step yields a line scaled by an Fq2 factor (killed by the final
// exponentiation), kept as (a, b, c): the line at P = (xP, yP) is a yP + b xP w + c w^3, sparse in positions c0.b0, c1.b0,
// c1.b1.  The final exponentiation is exactly (q^12 - 1) / r: the easy part (q^6 - 1)(q^2 + 1), then the hard part
// (q^4 - q^2 + 1) / r by Scott et al.'s addition chain in f^x, f^(x^2), f^(x^3) (x = 4965661367192848881), which computes
// that exponent itself and not a multiple of it.
#pragma once
#include "bn254_points_gfx950.hpp"  // and with it the generated constants (fq12_consts_gfx950.inc)

namespace cwc_g16 {

constexpr uint64_t BN_X = 4965661367192848881ull;  // the BN parameter x (63 bits)
// 6x + 2 = 2^64 + ATE_LOW: 65 bits; the Miller loop starts at T = Q for the top bit and walks bits 63 .. 0
constexpr uint64_t ATE_LOW = 0x9d797039be763ba8ull;
constexpr uint32_t ATE_ADDS = 36;                   // one bits among bits 63 .. 0 of 6x + 2
constexpr uint32_t N_LINES = 64 + ATE_ADDS + 2;      // lines of one Miller loop (doublings, additions, the two final ones)

// a / 2 mod q
FRD Fq fq_half(const Fq& a) {
    Fq t;
    cwc::u256_add(t, a, fq_p());  // < 2^255
    const Fq s = cwc::u256_select((a.v[0] & 1u) != 0u, t, a);
    Fq r;
#pragma unroll
    for (int i = 0; i < 8; ++i) r.v[i] = (s.v[i] >> 1) | (i < 7 ? s.v[i < 7 ? i + 1 : 7] << 31 : 0u);
    return r;
}

FRD Fq2 fq2_conj(const Fq2& a) { return Fq2{a.c0, fq_neg(a.c1)}; }
FRD Fq2 fq2_mul_fq(const Fq2& a, const Fq& s) { return Fq2{fq_mul(a.c0, s), fq_mul(a.c1, s)}; }
FRD Fq2 fq2_half(const Fq2& a) { return Fq2{fq_half(a.c0), fq_half(a.c1)}; }
FRD Fq2 fq2_zero() { return Fq2{fq_zero(), fq_zero()}; }
FRD Fq2 fq2_one() { return Fq2{fq_one(), fq_zero()}; }
// (a0 + a1 u)(9 + u) = 9 a0 - a1 + (a0 + 9 a1) u
FRD Fq2 fq2_mul_xi(const Fq2& a) {
    const Fq e0 = fq_dbl(fq_dbl(fq_dbl(a.c0))), e1 = fq_dbl(fq_dbl(fq_dbl(a.c1)));
    return Fq2{fq_sub(fq_add(e0, a.c0), a.c1), fq_add(fq_add(e1, a.c1), a.c0)};
}
FRD bool fq2_eq(const Fq2& a, const Fq2& b) { return Fq2T::eq(a, b); }

// ---- Fq6 -----------------------------------------------------------------------------------------------------------------------
struct Fq6 {
    Fq2 b0, b1, b2;
};

FRD Fq6 fq6_add(const Fq6& a, const Fq6& b) { return Fq6{fq2_add(a.b0, b.b0), fq2_add(a.b1, b.b1), fq2_add(a.b2, b.b2)}; }
FRD Fq6 fq6_sub(const Fq6& a, const Fq6& b) { return Fq6{fq2_sub(a.b0, b.b0), fq2_sub(a.b1, b.b1), fq2_sub(a.b2, b.b2)}; }
FRD Fq6 fq6_neg(const Fq6& a) { return Fq6{fq2_neg(a.b0), fq2_neg(a.b1), fq2_neg(a.b2)}; }
FRD Fq6 fq6_dbl(const Fq6& a) { return Fq6{fq2_dbl(a.b0), fq2_dbl(a.b1), fq2_dbl(a.b2)}; }
// a v = xi a2 + a0 v + a1 v^2
FRD Fq6 fq6_mul_v(const Fq6& a) { return Fq6{fq2_mul_xi(a.b2), a.b0, a.b1}; }
FRD Fq6 fq6_mul_fq2(const Fq6& a, const Fq2& s) { return Fq6{fq2_mul(a.b0, s), fq2_mul(a.b1, s), fq2_mul(a.b2, s)}; }
// Karatsuba: six Fq2 products
FRD Fq6 fq6_mul(const Fq6& a, const Fq6& b) {
    const Fq2 v0 = fq2_mul(a.b0, b.b0), v1 = fq2_mul(a.b1, b.b1), v2 = fq2_mul(a.b2, b.b2);
    const Fq2 t0 = fq2_sub(fq2_sub(fq2_mul(fq2_add(a.b1, a.b2), fq2_add(b.b1, b.b2)), v1), v2);
    const Fq2 t1 = fq2_sub(fq2_sub(fq2_mul(fq2_add(a.b0, a.b1), fq2_add(b.b0, b.b1)), v0), v1);
    const Fq2 t2 = fq2_sub(fq2_sub(fq2_mul(fq2_add(a.b0, a.b2), fq2_add(b.b0, b.b2)), v0), v2);
    return Fq6{fq2_add(v0, fq2_mul_xi(t0)), fq2_add(t1, fq2_mul_xi(v2)), fq2_add(t2, v1)};
}
// a (s0 + s1 v): five Fq2 products
FRD Fq6 fq6_mul_01(const Fq6& a, const Fq2& s0, const Fq2& s1) {
    const Fq2 v0 = fq2_mul(a.b0, s0), v1 = fq2_mul(a.b1, s1);
    const Fq2 c1 = fq2_sub(fq2_sub(fq2_mul(fq2_add(a.b0, a.b1), fq2_add(s0, s1)), v0), v1);
    return Fq6{fq2_add(v0, fq2_mul_xi(fq2_mul(a.b2, s1))), c1, fq2_add(v1, fq2_mul(a.b2, s0))};
}
FRD Fq6 fq6_inv(const Fq6& a) {
    const Fq2 t0 = fq2_sub(fq2_sqr(a.b0), fq2_mul_xi(fq2_mul(a.b1, a.b2)));
    const Fq2 t1 = fq2_sub(fq2_mul_xi(fq2_sqr(a.b2)), fq2_mul(a.b0, a.b1));
    const Fq2 t2 = fq2_sub(fq2_sqr(a.b1), fq2_mul(a.b0, a.b2));
    const Fq2 det = fq2_add(fq2_mul(a.b0, t0), fq2_mul_xi(fq2_add(fq2_mul(a.b2, t1), fq2_mul(a.b1, t2))));
    const Fq2 di = fq2_inv(det);
    return Fq6{fq2_mul(t0, di), fq2_mul(t1, di), fq2_mul(t2, di)};
}

// ---- Fq12 ----------------------------------------------------------------------------------------------------------------------
struct Fq12 {
    Fq6 c0, c1;
};

FRD Fq12 fq12_one() { return Fq12{Fq6{fq2_one(), fq2_zero(), fq2_zero()}, Fq6{fq2_zero(), fq2_zero(), fq2_zero()}}; }
FRD Fq12 fq12_conj(const Fq12& a) { return Fq12{a.c0, fq6_neg(a.c1)}; }
// Karatsuba: three Fq6 products
FRD Fq12 fq12_mul(const Fq12& a, const Fq12& b) {
    const Fq6 t0 = fq6_mul(a.c0, b.c0), t1 = fq6_mul(a.c1, b.c1);
    const Fq6 c1 = fq6_sub(fq6_sub(fq6_mul(fq6_add(a.c0, a.c1), fq6_add(b.c0, b.c1)), t0), t1);
    return Fq12{fq6_add(t0, fq6_mul_v(t1)), c1};
}
// complex squaring: (a0 + a1 w)^2 = (a0 + a1)(a0 + a1 v) - t - t v + 2 t w, t = a0 a1; two Fq6 products
FRD Fq12 fq12_sqr(const Fq12& a) {
    const Fq6 t = fq6_mul(a.c0, a.c1);
    const Fq6 c0 = fq6_sub(fq6_sub(fq6_mul(fq6_add(a.c0, a.c1), fq6_add(a.c0, fq6_mul_v(a.c1))), t), fq6_mul_v(t));
    return Fq12{c0, fq6_dbl(t)};
}
// 1 / (c0 + c1 w) = (c0 - c1 w) / (c0^2 - c1^2 v)
FRD Fq12 fq12_inv(const Fq12& a) {
    const Fq6 d = fq6_inv(fq6_sub(fq6_mul(a.c0, a.c0), fq6_mul_v(fq6_mul(a.c1, a.c1))));
    return Fq12{fq6_mul(a.c0, d), fq6_neg(fq6_mul(a.c1, d))};
}
FRD bool fq12_eq(const Fq12& a, const Fq12& b) {
    return cwc::both(cwc::both(cwc::both(fq2_eq(a.c0.b0, b.c0.b0), fq2_eq(a.c0.b1, b.c0.b1)), cwc::both(fq2_eq(a.c0.b2, b.c0.b2), fq2_eq(a.c1.b0, b.c1.b0))),
                     cwc::both(fq2_eq(a.c1.b1, b.c1.b1), fq2_eq(a.c1.b2, b.c1.b2)));
}

// f (l0 + l1 w + l3 w^3) = f (L0 + L1 w), L0 = (l0, 0, 0), L1 = (l1, l3, 0): 13 Fq2 products (a line of the Miller loop)
FRD Fq12 fq12_mul_line(const Fq12& f, const Fq2& l0, const Fq2& l1, const Fq2& l3) {
    const Fq6 t0 = fq6_mul_fq2(f.c0, l0), t1 = fq6_mul_01(f.c1, l1, l3);
    const Fq6 c1 = fq6_sub(fq6_sub(fq6_mul_01(fq6_add(f.c0, f.c1), fq2_add(l0, l1), l3), t0), t1);
    return Fq12{fq6_add(t0, fq6_mul_v(t1)), c1};
}

// f^(q^k) for k in 1 .. 3 chosen at run time (one code path; the final exponentiation's program picks k)
FRD Fq2 frob_const(uint32_t k, const Fq2& c1, const Fq2& c2, const Fq2& c3) {
    return Fq2{cwc::u256_select(k == 1, c1.c0, cwc::u256_select(k == 2, c2.c0, c3.c0)), cwc::u256_select(k == 1, c1.c1, cwc::u256_select(k == 2, c2.c1, c3.c1))};
}
FRD Fq12 fq12_frob(const Fq12& a, uint32_t k) {
    auto g = [&](const Fq2& x) { return (k & 1u) ? fq2_conj(x) : x; };
    return Fq12{Fq6{g(a.c0.b0), fq2_mul(g(a.c0.b1), frob_const(k, frob1_2(), frob2_2(), frob3_2())),
                    fq2_mul(g(a.c0.b2), frob_const(k, frob1_4(), frob2_4(), frob3_4()))},
                Fq6{fq2_mul(g(a.c1.b0), frob_const(k, frob1_1(), frob2_1(), frob3_1())),
                    fq2_mul(g(a.c1.b1), frob_const(k, frob1_3(), frob2_3(), frob3_3())),
                    fq2_mul(g(a.c1.b2), frob_const(k, frob1_5(), frob2_5(), frob3_5()))}};
}

// Granger-Scott squaring in the cyclotomic subgroup (elements after the easy part): the pairs (g0, g3), (g1, g4), (g2, g5)
// are squared in Fq4 = Fq2[w^3]/(w^6 - xi); nine Fq2 products' worth of work against twelve for fq12_sqr
FRD Fq2 csq_t(const Fq2& x, const Fq2& y, Fq2& t1) {  // (x + y s)^2 in Fq4 (s^2 = xi): returns the 1-part, t1 = the s-part
    const Fq2 p = fq2_mul(x, y);
    t1 = fq2_dbl(p);
    return fq2_sub(fq2_sub(fq2_mul(fq2_add(x, y), fq2_add(fq2_mul_xi(y), x)), p), fq2_mul_xi(p));
}
FRD Fq2 thrice_minus_twice(const Fq2& t, const Fq2& z) { const Fq2 d = fq2_sub(t, z); return fq2_add(fq2_dbl(d), t); }  // 3t - 2z
FRD Fq2 thrice_plus_twice(const Fq2& t, const Fq2& z) { const Fq2 d = fq2_add(t, z); return fq2_add(fq2_dbl(d), t); }   // 3t + 2z
FRD Fq12 fq12_cyclotomic_sqr(const Fq12& a) {
    Fq2 t1, t3, t5;
    const Fq2 t0 = csq_t(a.c0.b0, a.c1.b1, t1);
    const Fq2 t2 = csq_t(a.c1.b0, a.c0.b2, t3);
    const Fq2 t4 = csq_t(a.c0.b1, a.c1.b2, t5);
    Fq12 r;
    r.c0.b0 = thrice_minus_twice(t0, a.c0.b0);
    r.c1.b1 = thrice_plus_twice(t1, a.c1.b1);
    r.c1.b0 = thrice_plus_twice(fq2_mul_xi(t5), a.c1.b0);
    r.c0.b2 = thrice_minus_twice(t4, a.c0.b2);
    r.c0.b1 = thrice_minus_twice(t2, a.c0.b1);
    r.c1.b2 = thrice_plus_twice(t3, a.c1.b2);
    return r;
}

// ---- the final exponentiation as a program ---------------------------------------------------------------------------------
// One accumulator in registers and numbered slots (spilled by the caller) run a fixed program, so that each Fq12 primitive has
// one call site in a kernel.  Op = kind << 4 | argument.
enum : uint8_t { FX_MUL = 0, FX_CSQ = 1, FX_FROB = 2, FX_CONJ = 3, FX_ST = 4, FX_LD = 5 };
constexpr uint32_t FX_SLOTS = 8;
struct FxProg {
    uint8_t op[512];
    uint32_t n;
};
// The hard part (q^4 - q^2 + 1) / r, applied to the easy part's result, by Scott et al.'s chain:
//   y0 = f^q f^(q^2) f^(q^3), y1 = 1/f, y2 = (f^(x^2))^(q^2), y3 = 1/(f^x)^q, y4 = 1/(f^x (f^(x^2))^q), y5 = 1/f^(x^2),
//   y6 = 1/(f^(x^3) (f^(x^3))^q);  T0 = y6^2 y4 y5, T1 = y3 y5 T0, T0 = T0 y2, T1 = (T1^2 T0)^2, result = (T1 y1)^2 T1 y0
// (inverses are conjugates in the cyclotomic subgroup).  Slots: 0 f, 1 f^x, 2 f^(x^2),
// 3 f^(x^3), 4 T0, 5 y5, 6 T1, 7 temporary.
constexpr FxProg fx_prog() {
    FxProg p{};
    p.n = 0;
    auto e = [&p](uint8_t kind, uint8_t arg) { p.op[p.n++] = (uint8_t)(kind << 4 | arg); };
    auto expx = [&](uint8_t base) {  // acc = S[base] -> S[base]^x
        for (int b = 61; b >= 0; --b) {
            e(FX_CSQ, 0);
            if ((BN_X >> b) & 1ull) e(FX_MUL, base);
        }
    };
    e(FX_ST, 0);
    expx(0), e(FX_ST, 1);
    expx(1), e(FX_ST, 2);
    expx(2), e(FX_ST, 3);
    e(FX_FROB, 1), e(FX_MUL, 3), e(FX_CONJ, 0), e(FX_CSQ, 0), e(FX_ST, 4);                 // y6^2
    e(FX_LD, 2), e(FX_FROB, 1), e(FX_MUL, 1), e(FX_CONJ, 0), e(FX_MUL, 4), e(FX_ST, 4);  // y6^2 y4
    e(FX_LD, 2), e(FX_CONJ, 0), e(FX_ST, 5), e(FX_MUL, 4), e(FX_ST, 4);                  // T0 = y6^2 y4 y5
    e(FX_LD, 1), e(FX_FROB, 1), e(FX_CONJ, 0), e(FX_MUL, 5), e(FX_MUL, 4), e(FX_ST, 6);  // T1 = y3 y5 T0
    e(FX_LD, 2), e(FX_FROB, 2), e(FX_MUL, 4), e(FX_ST, 4);                               // T0 = T0 y2
    e(FX_LD, 6), e(FX_CSQ, 0), e(FX_MUL, 4), e(FX_CSQ, 0), e(FX_ST, 6);                  // T1 = (T1^2 T0)^2
    e(FX_LD, 0), e(FX_CONJ, 0), e(FX_MUL, 6), e(FX_ST, 4);                               // T0 = T1 y1
    e(FX_LD, 0), e(FX_FROB, 1), e(FX_ST, 7), e(FX_LD, 0), e(FX_FROB, 2), e(FX_MUL, 7), e(FX_ST, 7);
    e(FX_LD, 0), e(FX_FROB, 3), e(FX_MUL, 7), e(FX_MUL, 6), e(FX_ST, 6);                 // T1 = T1 y0
    e(FX_LD, 4), e(FX_CSQ, 0), e(FX_MUL, 6);                                            // T0^2 T1
    return p;
}

// the easy part f^((q^6 - 1)(q^2 + 1)) = (conj(f) / f)^(q^2 + 1), f != 0; f() yields the Miller value (a kernel reloads it
// rather than keep it live across the inversion)
template <class Load>
FRD Fq12 final_exp_easy(Load&& f) {
    Fq12 t = fq12_inv(f());
    t = fq12_mul(t, fq12_conj(f()));
    return fq12_mul(fq12_frob(t, 2), t);
}

// the hard part by the program on the easy part's result; spill(slot, value) / fill(slot) hold the slots
template <class Spill, class Fill>
FRD Fq12 final_exp_run(const FxProg& prog, Fq12 acc, Spill&& spill, Fill&& fill) {
    for (uint32_t pc = 0; pc < prog.n; ++pc) {
        const uint32_t kind = prog.op[pc] >> 4, arg = prog.op[pc] & 15u;
        if (kind == FX_MUL) acc = fq12_mul(acc, fill(arg));
        else if (kind == FX_CSQ) acc = fq12_cyclotomic_sqr(acc);
        else if (kind == FX_FROB) acc = fq12_frob(acc, arg);
        else if (kind == FX_CONJ) acc = fq12_conj(acc);
        else if (kind == FX_ST) spill(arg, acc);
        else acc = fill(arg);
    }
    return acc;
}

// ---- G2 lines ------------------------------------------------------------------------------------------------------------------
struct Line {
    Fq2 a, b, c;  // a yP + b xP w + c w^3
};
struct G2Proj {
    Fq2 X, Y, Z;
};

// T <- 2T; the tangent at T: -2YZ yP + 3X^2 xP w + (3b'Z^2 - Y^2) w^3
FRD Line g2_dbl_step(G2Proj& T) {
    const Fq2 a = fq2_half(fq2_mul(T.X, T.Y)), b = fq2_sqr(T.Y), c = fq2_sqr(T.Z);
    const Fq2 e = fq2_mul(twist_b3(), c);  // 3b'Z^2
    const Fq2 f = fq2_add(fq2_dbl(e), e);   // 9b'Z^2
    const Fq2 g = fq2_half(fq2_add(b, f));
    const Fq2 h = fq2_sub(fq2_sqr(fq2_add(T.Y, T.Z)), fq2_add(b, c));  // 2YZ
    const Fq2 j = fq2_sqr(T.X);
    const Fq2 e2 = fq2_sqr(e);
    const Line l{fq2_neg(h), fq2_add(fq2_dbl(j), j), fq2_sub(e, b)};
    T.X = fq2_mul(a, fq2_sub(b, f));
    T.Y = fq2_sub(fq2_sqr(g), fq2_add(fq2_dbl(e2), e2));
    T.Z = fq2_mul(b, h);
    return l;
}

// T <- T + Q (affine Q); the line through T and Q: lambda yP - theta xP w + (theta xQ - lambda yQ) w^3
FRD Line g2_add_step(G2Proj& T, const Fq2& qx, const Fq2& qy) {
    const Fq2 theta = fq2_sub(T.Y, fq2_mul(qy, T.Z)), lambda = fq2_sub(T.X, fq2_mul(qx, T.Z));
    const Fq2 c = fq2_sqr(theta), d = fq2_sqr(lambda);
    const Fq2 e = fq2_mul(lambda, d), f = fq2_mul(T.Z, c), g = fq2_mul(T.X, d);
    const Fq2 h = fq2_sub(fq2_add(e, f), fq2_dbl(g));
    const Line l{lambda, fq2_neg(theta), fq2_sub(fq2_mul(theta, qx), fq2_mul(lambda, qy))};
    T.X = fq2_mul(lambda, h);
    T.Y = fq2_sub(fq2_mul(theta, fq2_sub(g, h)), fq2_mul(e, T.Y));
    T.Z = fq2_mul(T.Z, e);
    return l;
}

FRD Fq12 fq12_mul_line_at(const Fq12& f, const Line& l, const Fq& xP, const Fq& yP) {
    return fq12_mul_line(f, fq2_mul_fq(l.a, yP), fq2_mul_fq(l.b, xP), l.c);
}

// pi(Q) and -pi^2(Q) on the twist (the final two points of the Miller loop)
FRD void g2_frob1(const Fq2& x, const Fq2& y, Fq2& ox, Fq2& oy) {
    ox = fq2_mul(fq2_conj(x), frob1_2());
    oy = fq2_mul(fq2_conj(y), frob1_3());
}
FRD void g2_neg_frob2(const Fq2& x, const Fq2& y, Fq2& ox, Fq2& oy) {
    ox = fq2_mul_fq(x, frob2_2().c0);
    oy = fq2_neg(fq2_mul_fq(y, frob2_3().c0));
}

// The Miller loop's schedule: step k is a doubling (0) or an addition of Q (1), pi(Q) (2) or -pi^2(Q) (3): bits 63 .. 0 of
// ATE_LOW (a doubling each, an addition after it for a one bit), then the two final additions.  Prepared keys store their
// lines in this order.
struct MillerSched {
    uint8_t kind[N_LINES];
};
constexpr MillerSched miller_sched() {
    MillerSched s{};
    uint32_t n = 0;
    for (int i = 63; i >= 0; --i) {
        s.kind[n++] = 0;
        if ((ATE_LOW >> i) & 1ull) s.kind[n++] = 1;
    }
    s.kind[n++] = 2;
    s.kind[n++] = 3;
    return s;
}

// one step of the schedule for T (started at Q): the line it yields
FRD Line miller_step(uint32_t kind, G2Proj& T, const Fq2& qx, const Fq2& qy) {
    if (kind == 0) return g2_dbl_step(T);
    Fq2 x = qx, y = qy;
    if (kind == 2) g2_frob1(qx, qy, x, y);
    if (kind == 3) g2_neg_frob2(qx, qy, x, y);
    return g2_add_step(T, x, y);
}

}  // namespace cwc_g16
