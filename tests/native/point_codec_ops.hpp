// One record of the point-codec tests: reads the operand words, runs one primitive of r1cs/point_codec_gfx950.hpp and writes the raw
// result words.  Shared by the device harness (point_codec.hip, one record per lane) and the host program (point_codec_host.cc, a
// loop); it holds no expected values: tests/point_codec_cases.py compares with Python integers.
//
// Records, operands -> results (words):
//   fq_sqrt a (8, Montgomery) -> root (8, Montgomery), verdict (1)      fq2_sqrt a (16) -> root (16), verdict (1)
//   fq_is_larger y (8, canonical) -> verdict (1)                         fq2_is_larger y (16) -> verdict (1)
//   g1_encode form (1), point (16) -> encoding (8)                       g2_encode form (1), point (32) -> encoding (16)
//   g1_decode form (1), encoding (8) -> point (16), status (1)           g2_decode form (1), encoding (16) -> point (32), status (1)
// form is 0 (canonical) or 1 (Montgomery), as GWB_FORM_*.
#pragma once
#include <stdint.h>

#include "point_codec_gfx950.hpp"

namespace codec_ops {
using namespace cwc_g16;

enum Op : uint32_t { OP_FQ_SQRT = 1, OP_FQ2_SQRT, OP_FQ_IS_LARGER, OP_FQ2_IS_LARGER, OP_G1_ENCODE, OP_G2_ENCODE, OP_G1_DECODE, OP_G2_DECODE, OP_END };

constexpr uint32_t GUARD = 64;            // guard records after every section's results
constexpr uint32_t MAX_RECORDS = 1u << 16;

constexpr uint32_t in_words(uint32_t op) {
    return op == OP_FQ_SQRT || op == OP_FQ_IS_LARGER ? 8 : op == OP_FQ2_SQRT || op == OP_FQ2_IS_LARGER ? 16 : op == OP_G1_ENCODE ? 17
         : op == OP_G2_ENCODE ? 33 : op == OP_G1_DECODE ? 9 : 17;
}
constexpr uint32_t out_words(uint32_t op) {
    return op == OP_FQ_SQRT ? 9 : op == OP_FQ2_SQRT ? 17 : op == OP_FQ_IS_LARGER || op == OP_FQ2_IS_LARGER ? 1 : op == OP_G1_ENCODE ? 8
         : op == OP_G2_ENCODE ? 16 : op == OP_G1_DECODE ? 17 : 33;
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

// r: in_words(OP) operand words, o: out_words(OP) result words
template <uint32_t OP>
FRD void run_record(const uint32_t* r, uint32_t* o) {
    static_assert(OP >= OP_FQ_SQRT && OP < OP_END, "unknown op");
    const uint8_t* rb = reinterpret_cast<const uint8_t*>(r + 1);  // the bytes behind a form word
    uint8_t* ob = reinterpret_cast<uint8_t*>(o);
    if constexpr (OP == OP_FQ_SQRT) {
        Fq root;
        const bool ok = fq_sqrt(ld<Fq>(r), root);
        st(o, root);
        o[8] = ok ? 1u : 0u;
    } else if constexpr (OP == OP_FQ2_SQRT) {
        Fq2 root;
        const bool ok = fq2_sqrt(ld<Fq2>(r), root);
        st(o, root);
        o[16] = ok ? 1u : 0u;
    } else if constexpr (OP == OP_FQ_IS_LARGER) {
        o[0] = fq_is_larger(ld<Fq>(r)) ? 1u : 0u;
    } else if constexpr (OP == OP_FQ2_IS_LARGER) {
        o[0] = fq2_is_larger(ld<Fq2>(r)) ? 1u : 0u;
    } else if constexpr (OP == OP_G1_ENCODE) {
        g1_encode(rb, r[0] == 0u, ob);
    } else if constexpr (OP == OP_G2_ENCODE) {
        g2_encode(rb, r[0] == 0u, ob);
    } else if constexpr (OP == OP_G1_DECODE) {
        o[16] = g1_decode(rb, r[0] == 0u, ob);
    } else {
        o[32] = g2_decode(rb, r[0] == 0u, ob);
    }
}

}  // namespace codec_ops
