// One record of the pairing-tower tests: reads the operand words, runs one primitive of r1cs/fq12_gfx950.hpp (or fq_gfx950.hpp) and
// writes the raw Montgomery result limbs.  Shared by the device harness (fq12_tower.hip, one record per lane) and the host program
// (fq12_tower_host.cc, a loop); it holds no expected values: tests/fq12_tower_cases.py compares with Python integers.
//
// Words per value: Fq 8, Fq2 16 (c0, c1), Fq6 48 (b0, b1, b2), Fq12 96 (c0, c1), a line 48 (a, b, c), a projective G2 point 48
// (X, Y, Z), an affine one 32 (x, y); k and kind are one word.  Records, operands in this order -> results:
//   fq_half a | fq2_half, fq2_sqr, fq2_inv, fq2_conj, fq2_mul_xi a | fq2_mul a b | fq2_mul_fq a s
//   fq6_mul a b | fq6_mul_01 a s0 s1 | fq6_mul_fq2 a s | fq6_mul_v, fq6_inv a
//   fq12_mul a b | fq12_sqr, fq12_inv, fq12_conj, fq12_cyclotomic_sqr, final_exp_easy, final_exp_run(fx_prog()) a
//   fq12_mul_line f l0 l1 l3 | fq12_mul_line_at f line xP yP | fq12_frob a k
//   g2_dbl_step T -> T, line | g2_add_step T q -> T, line | miller_step kind T q -> T, line | g2_frob1, g2_neg_frob2 q -> q
#pragma once
#include <stdint.h>

#include "fq12_gfx950.hpp"

namespace tower_ops {
using namespace cwc_g16;

enum Op : uint32_t {
    OP_FQ_HALF = 1, OP_FQ2_HALF, OP_FQ2_MUL, OP_FQ2_SQR, OP_FQ2_INV, OP_FQ2_CONJ, OP_FQ2_MUL_FQ, OP_FQ2_MUL_XI,
    OP_FQ6_MUL, OP_FQ6_MUL_01, OP_FQ6_MUL_FQ2, OP_FQ6_MUL_V, OP_FQ6_INV,
    OP_FQ12_MUL, OP_FQ12_SQR, OP_FQ12_INV, OP_FQ12_CONJ, OP_FQ12_MUL_LINE, OP_FQ12_MUL_LINE_AT, OP_FQ12_FROB, OP_FQ12_CSQ,
    OP_FINAL_EASY, OP_FINAL_HARD,
    OP_G2_DBL_STEP, OP_G2_ADD_STEP, OP_G2_FROB1, OP_G2_NEG_FROB2, OP_MILLER_STEP,
    OP_END
};

constexpr uint32_t SLOT_WORDS = FX_SLOTS * 96;  // the FxProg slots of one record, slot s at words [96 s, 96 s + 96)

constexpr uint32_t in_words(uint32_t op) {
    return op == OP_FQ_HALF ? 8
         : op == OP_FQ2_MUL || op == OP_G2_FROB1 || op == OP_G2_NEG_FROB2 ? 32
         : op == OP_FQ2_MUL_FQ ? 24
         : op >= OP_FQ2_HALF && op <= OP_FQ2_MUL_XI ? 16
         : op == OP_FQ6_MUL ? 96 : op == OP_FQ6_MUL_01 ? 80 : op == OP_FQ6_MUL_FQ2 ? 64 : op == OP_FQ6_MUL_V || op == OP_FQ6_INV ? 48
         : op == OP_FQ12_MUL ? 192 : op == OP_FQ12_MUL_LINE ? 144 : op == OP_FQ12_MUL_LINE_AT ? 160 : op == OP_FQ12_FROB ? 97
         : op == OP_G2_DBL_STEP ? 48 : op == OP_G2_ADD_STEP ? 80 : op == OP_MILLER_STEP ? 81 : 96;
}
constexpr uint32_t out_words(uint32_t op) {
    return op == OP_FQ_HALF ? 8 : op <= OP_FQ2_MUL_XI ? 16 : op <= OP_FQ6_INV ? 48 : op == OP_G2_FROB1 || op == OP_G2_NEG_FROB2 ? 32 : 96;
}

template <class X>
FRD X ld(const uint32_t* p) {
    static_assert(sizeof(X) % 4 == 0, "whole words");
    X v;
    uint32_t* w = reinterpret_cast<uint32_t*>(&v);
    for (uint32_t k = 0; k < sizeof(X) / 4; ++k) w[k] = p[k];
    return v;
}
template <class X>
FRD void st(uint32_t* p, const X& v) {
    const uint32_t* w = reinterpret_cast<const uint32_t*>(&v);
    for (uint32_t k = 0; k < sizeof(X) / 4; ++k) p[k] = w[k];
}
// the slots are written and read where the program says (volatile: as the verifier's spill buffer)
FRD void st_slot(uint32_t* p, const Fq12& v) {
    const uint32_t* w = reinterpret_cast<const uint32_t*>(&v);
    volatile uint32_t* b = p;
    for (uint32_t k = 0; k < 96; ++k) b[k] = w[k];
}
FRD Fq12 ld_slot(const uint32_t* p) {
    Fq12 v;
    uint32_t* w = reinterpret_cast<uint32_t*>(&v);
    const volatile uint32_t* b = p;
    for (uint32_t k = 0; k < 96; ++k) w[k] = b[k];
    return v;
}

FRD void st_step(uint32_t* o, const G2Proj& T, const Line& l) {
    st(o, T);
    st(o + 48, l);
}

// r: in_words(OP) operand words, o: out_words(OP) result words, slots: SLOT_WORDS words of this record's own (OP_FINAL_HARD only)
template <uint32_t OP>
FRD void run_record(const uint32_t* r, uint32_t* o, const FxProg& prog, uint32_t* slots) {
    static_assert(OP >= OP_FQ_HALF && OP < OP_END, "unknown op");
    if constexpr (OP == OP_FQ_HALF) st(o, fq_half(ld<Fq>(r)));
    if constexpr (OP == OP_FQ2_HALF) st(o, fq2_half(ld<Fq2>(r)));
    if constexpr (OP == OP_FQ2_MUL) st(o, fq2_mul(ld<Fq2>(r), ld<Fq2>(r + 16)));
    if constexpr (OP == OP_FQ2_SQR) st(o, fq2_sqr(ld<Fq2>(r)));
    if constexpr (OP == OP_FQ2_INV) st(o, fq2_inv(ld<Fq2>(r)));
    if constexpr (OP == OP_FQ2_CONJ) st(o, fq2_conj(ld<Fq2>(r)));
    if constexpr (OP == OP_FQ2_MUL_FQ) st(o, fq2_mul_fq(ld<Fq2>(r), ld<Fq>(r + 16)));
    if constexpr (OP == OP_FQ2_MUL_XI) st(o, fq2_mul_xi(ld<Fq2>(r)));
    if constexpr (OP == OP_FQ6_MUL) st(o, fq6_mul(ld<Fq6>(r), ld<Fq6>(r + 48)));
    if constexpr (OP == OP_FQ6_MUL_01) st(o, fq6_mul_01(ld<Fq6>(r), ld<Fq2>(r + 48), ld<Fq2>(r + 64)));
    if constexpr (OP == OP_FQ6_MUL_FQ2) st(o, fq6_mul_fq2(ld<Fq6>(r), ld<Fq2>(r + 48)));
    if constexpr (OP == OP_FQ6_MUL_V) st(o, fq6_mul_v(ld<Fq6>(r)));
    if constexpr (OP == OP_FQ6_INV) st(o, fq6_inv(ld<Fq6>(r)));
    if constexpr (OP == OP_FQ12_MUL) st(o, fq12_mul(ld<Fq12>(r), ld<Fq12>(r + 96)));
    if constexpr (OP == OP_FQ12_SQR) st(o, fq12_sqr(ld<Fq12>(r)));
    if constexpr (OP == OP_FQ12_INV) st(o, fq12_inv(ld<Fq12>(r)));
    if constexpr (OP == OP_FQ12_CONJ) st(o, fq12_conj(ld<Fq12>(r)));
    if constexpr (OP == OP_FQ12_MUL_LINE) st(o, fq12_mul_line(ld<Fq12>(r), ld<Fq2>(r + 96), ld<Fq2>(r + 112), ld<Fq2>(r + 128)));
    if constexpr (OP == OP_FQ12_MUL_LINE_AT) st(o, fq12_mul_line_at(ld<Fq12>(r), ld<Line>(r + 96), ld<Fq>(r + 144), ld<Fq>(r + 152)));
    if constexpr (OP == OP_FQ12_FROB) st(o, fq12_frob(ld<Fq12>(r), r[96]));
    if constexpr (OP == OP_FQ12_CSQ) st(o, fq12_cyclotomic_sqr(ld<Fq12>(r)));
    if constexpr (OP == OP_FINAL_EASY) st(o, final_exp_easy([&] { return ld_slot(r); }));
    if constexpr (OP == OP_FINAL_HARD)
        st(o, final_exp_run(prog, ld<Fq12>(r), [&](uint32_t s, const Fq12& v) { st_slot(slots + 96 * s, v); },
                            [&](uint32_t s) { return ld_slot(slots + 96 * s); }));
    if constexpr (OP == OP_G2_DBL_STEP) {
        G2Proj T = ld<G2Proj>(r);
        const Line l = g2_dbl_step(T);
        st_step(o, T, l);
    }
    if constexpr (OP == OP_G2_ADD_STEP) {
        G2Proj T = ld<G2Proj>(r);
        const Line l = g2_add_step(T, ld<Fq2>(r + 48), ld<Fq2>(r + 64));
        st_step(o, T, l);
    }
    if constexpr (OP == OP_MILLER_STEP) {
        G2Proj T = ld<G2Proj>(r + 1);
        const Line l = miller_step(r[0], T, ld<Fq2>(r + 49), ld<Fq2>(r + 65));
        st_step(o, T, l);
    }
    if constexpr (OP == OP_G2_FROB1 || OP == OP_G2_NEG_FROB2) {
        Fq2 x, y;
        if constexpr (OP == OP_G2_FROB1) g2_frob1(ld<Fq2>(r), ld<Fq2>(r + 16), x, y);
        if constexpr (OP == OP_G2_NEG_FROB2) g2_neg_frob2(ld<Fq2>(r), ld<Fq2>(r + 16), x, y);
        st(o, x);
        st(o + 16, y);
    }
}

// the section files of both programs: { u32 op, n, in_words, out_words, param; u32 data[n * in_words] } back to back (param is
// unused and zero); the results back to back, per section (n + GUARD) * out_words words: the last GUARD records belong to no
// record and must come back as they were filled (0xa5 bytes)
constexpr uint32_t GUARD = 64;
constexpr uint32_t MAX_RECORDS = 1u << 16;

}  // namespace tower_ops
