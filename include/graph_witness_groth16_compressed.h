/* Compressed BN254 points, Groth16 proofs and verifying keys, coded and decoded on an MI355X: the byte form that arkworks
 * provers and verifiers (ark-groth16, ark-circom and what is built on them) exchange, beside snarkjs's uncompressed form that
 * the rest of the library speaks.  The symbols are in libcwc_r1cs.so.
 *
 * The format is arkworks 0.4 CanonicalSerialize with Compress::Yes, restated from memory and checked against hand-computed
 * anchors only (no arkworks build was at hand):
 *   G1 point, 32 B   x, canonical little-endian; flags in the top two bits of byte 31 (q < 2^254 leaves them free)
 *   G2 point, 64 B   x.c0 then x.c1, 32 B each; flags in the top two bits of byte 63
 *   flag 0x40        the point at infinity; every other bit of the encoding is zero
 *   flag 0x80        y is the larger of y and -y: for Fq, y > q - y as canonical integers; for Fq2, y.c1 > q - y.c1 when
 *                    y.c1 != 0, else y.c0 > q - y.c0 (c1 first).  No flag: the smaller one.
 *   proof, 128 B     A (32) B (64) C (32)                                    GWB_GROTH16_CPROOF_BYTES
 *   key              alpha1 (32) beta2 (64) gamma2 (64) delta2 (64) u64le(nPublic + 1) IC_0 .. IC_nPublic (32 each):
 *                    232 + 32 (nPublic + 1) bytes
 * Anchors: (1, 2) is 01 00 .. 00; -(1, 2) is 01 00 .. 00 80; infinity is 00 .. 00 40; the G2 generator has y.c1 below
 * (q - 1) / 2 and is x.c0, x.c1 with no flag.
 *
 * Decoding is strict.  An encoding is refused (status GWB_G16V_POINT, and the point (0, 0) is written) when both flags are
 * set, when the infinity flag stands beside any other nonzero bit (arkworks ignores x there; this library does not), when a
 * coordinate with the flags masked off is >= q, when x^3 + b has no square root (b = 3, or 3 / (9 + u) on the twist), and for
 * flag 0x80 with y = 0 (no such point exists).  A decoded point lies on its curve by construction; membership of G2's order-r
 * subgroup stays what the verifier checks.  Encoding does not validate: points are below q and on their curves, or all zero
 * (infinity), as for gwb_bn254_pairing_batch_device.
 *
 * Uncompressed points are those of graph_witness_groth16_verify.h (G1 64 B, G2 128 B, zero bytes = infinity) in form
 * GWB_FORM_CANONICAL or GWB_FORM_MONTGOMERY; compressed bytes are always canonical.  group is 1 (G1) or 2 (G2).  Return and
 * status conventions are those of graph_witness_r1cs.h (0 on success, 1 on failure with status filled); an unknown group or
 * form returns 1 before any device work; n = 0 does nothing.  Device calls are asynchronous on hip_stream; what they need
 * beyond their arguments is allocated and freed in stream order. */
#ifndef CWC_AMD_GRAPH_WITNESS_GROTH16_COMPRESSED_H
#define CWC_AMD_GRAPH_WITNESS_GROTH16_COMPRESSED_H

#include <stddef.h>
#include <stdint.h>

#include "graph_witness_groth16_verify.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GWB_G1_COMPRESSED_BYTES 32
#define GWB_G2_COMPRESSED_BYTES 64
#define GWB_GROTH16_CPROOF_BYTES 128
#define GWB_G16VK_COMPRESSED_BYTES(n_public) (232 + 32 * ((size_t)(n_public) + 1))

/* d_points [n] (64 B or 128 B each, in `form`) -> d_out [n] (32 B or 64 B each). */
int gwb_bn254_compress_batch_device(const void *d_points, size_t n, uint32_t group, uint32_t form, void *d_out, void *hip_stream,
                                    gw_status_t *status);
/* d_in [n] (32 B or 64 B each) -> d_points [n] in `form` and d_status [n] uint32: GWB_G16V_VALID, or GWB_G16V_POINT beside
 * the point (0, 0). */
int gwb_bn254_decompress_batch_device(const void *d_in, size_t n, uint32_t group, uint32_t form, void *d_points, void *d_status,
                                      void *hip_stream, gw_status_t *status);
/* Device proofs [batch][256 B] (the prover's layout, canonical) -> d_out [batch][128 B]. */
int gwb_groth16_proofs_compress_device(const void *d_proofs, size_t batch, void *d_out, void *hip_stream, gw_status_t *status);
/* Device d_in [batch][128 B] -> d_proofs [batch][256 B] and d_status [batch] uint32: GWB_G16V_POINT when any of A, B, C was
 * refused (that point is then (0, 0)), else GWB_G16V_VALID. */
int gwb_groth16_proofs_decompress_device(const void *d_in, size_t batch, void *d_proofs, void *d_status, void *hip_stream,
                                         gw_status_t *status);

/* gwb_groth16_verify_batch_device on compressed proofs [batch][128 B].  The statuses and their order are the raw call's
 * (PUBLIC, POINT, SUBGROUP, EQUATION): a row with a refused encoding is GWB_G16V_POINT unless a public signal >= r makes it
 * GWB_G16V_PUBLIC.  Same stream rule as the raw call (the key's workspace is shared). */
int gwb_groth16_verify_batch_compressed_device(gwb_g16vk_t *vk, const void *d_cproofs, const void *d_public, size_t n_public, size_t batch,
                                               void *d_status, void *hip_stream, gw_status_t *status);
/* The same with host arrays; synchronous. */
int gwb_groth16_verify_batch_compressed_host(gwb_g16vk_t *vk, const void *cproofs, const void *pub, size_t n_public, size_t batch,
                                             void *status_out, gw_status_t *status);

/* A key from its compressed bytes, decoded on the host (once per key).  Refusals start "verifying key:": a length that is not
 * 232 + 32 k for a k >= 1, a length prefix that disagrees with the byte count, a refused encoding (the point is named: alpha1,
 * beta2, gamma2, delta2, IC[i]), then whatever gwb_g16vk_load refuses. */
int gwb_g16vk_load_compressed(const void *bytes, size_t len, gwb_g16vk_t **out, gw_status_t *status);
/* The key's compressed bytes; len must be GWB_G16VK_COMPRESSED_BYTES(nPublic).  Returns 1 on a NULL or a wrong len. */
int gwb_g16vk_compressed(const gwb_g16vk_t *vk, void *out, size_t len);

#ifdef __cplusplus
}
#endif
#endif /* CWC_AMD_GRAPH_WITNESS_GROTH16_COMPRESSED_H */
