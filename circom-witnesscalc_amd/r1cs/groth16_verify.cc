// groth16-verify <verification_key.json> <public.json> <proof.json>: checks a Groth16 proof on the GPU (snarkjs `groth16
// verify`, same argument order).  Exit status 0 and "OK!" for a valid proof; 1 and the failing status (PUBLIC, POINT,
// SUBGROUP, EQUATION) for an invalid one; 2 on a usage, file, JSON or format error.  Every input is parsed, and the key
// validated, before the device is touched.
//
// Shapes (snarkjs's): the key {"protocol": "groth16", "curve": "bn128", "nPublic": n, "vk_alpha_1": [x, y, z],
// "vk_beta_2": [[x0, x1], [y0, y1], [z0, z1]], "vk_gamma_2", "vk_delta_2", "IC": [[x, y, z] x (n + 1)], ...}
// (vk_alphabeta_12 and other members ignored); the proof {"pi_a", "pi_b", "pi_c"} alike; public signals a list of decimal
// strings.  z is "1" for an affine point and "0" for the point at infinity (proof_json's convention); numbers are decimal
// strings (or JSON integers) below 2^256.
//
// groth16-verify --compressed <vk.bin> <public.json> <proof.bin> (the flag first) takes the key and the proof in arkworks'
// compressed bytes (include/graph_witness_groth16_compressed.h: 232 + 32 (nPublic + 1) and 128 bytes); public.json is the same.
// A proof file of another size, or a key that strict decoding refuses, is exit status 2; a proof whose encoding is refused is
// INVALID: POINT.
#include <map>

#include "../../include/graph_witness_groth16_compressed.h"
#include "../../include/graph_witness_groth16_verify.h"
#include "cli_common.hpp"

namespace {

using Vk = cli::Owned<gwb_g16vk_t, gwb_g16vk_free>;

struct Bad {
    std::string msg;
};

struct J {  // a JSON value: kind 's' string, 'n' number (text kept), 'a' array, 'o' object, 'l' literal
    char kind = 'l';
    std::string text;
    std::vector<J> items;
    std::map<std::string, J> members;
};

struct Parser {
    const std::string& s;
    size_t i = 0;
    void ws() {
        while (i < s.size() && (s[i] == ' ' || s[i] == '\n' || s[i] == '\r' || s[i] == '\t')) ++i;
    }
    [[noreturn]] void fail(const char* what) { throw Bad{std::string("JSON: ") + what + " at offset " + std::to_string(i)}; }
    J value(int depth) {
        if (depth > 64) fail("nesting too deep");
        ws();
        if (i >= s.size()) fail("unexpected end");
        J v;
        const char c = s[i];
        if (c == '"') {
            v.kind = 's';
            for (++i; i < s.size() && s[i] != '"'; ++i) {
                if (s[i] == '\\') fail("escapes are not supported");
                v.text += s[i];
            }
            if (i >= s.size()) fail("unterminated string");
            ++i;
        } else if (c == '[') {
            v.kind = 'a';
            ++i;
            ws();
            if (i < s.size() && s[i] == ']') {
                ++i;
                return v;
            }
            for (;;) {
                v.items.push_back(value(depth + 1));
                ws();
                if (i < s.size() && s[i] == ',') {
                    ++i;
                    continue;
                }
                if (i < s.size() && s[i] == ']') {
                    ++i;
                    break;
                }
                fail("expected , or ]");
            }
        } else if (c == '{') {
            v.kind = 'o';
            ++i;
            ws();
            if (i < s.size() && s[i] == '}') {
                ++i;
                return v;
            }
            for (;;) {
                ws();
                const J k = value(depth + 1);
                if (k.kind != 's') fail("expected a member name");
                ws();
                if (i >= s.size() || s[i] != ':') fail("expected :");
                ++i;
                v.members[k.text] = value(depth + 1);
                ws();
                if (i < s.size() && s[i] == ',') {
                    ++i;
                    continue;
                }
                if (i < s.size() && s[i] == '}') {
                    ++i;
                    break;
                }
                fail("expected , or }");
            }
        } else if ((c >= '0' && c <= '9') || c == '-') {
            v.kind = 'n';
            while (i < s.size() && (isdigit((unsigned char)s[i]) || strchr("-+.eE", s[i]))) v.text += s[i++];
        } else {
            for (const char* lit : {"true", "false", "null"})
                if (s.compare(i, strlen(lit), lit) == 0) {
                    i += strlen(lit);
                    v.text = lit;
                    return v;
                }
            fail("unexpected character");
        }
        return v;
    }
    J parse() {
        J v = value(0);
        ws();
        if (i != s.size()) fail("trailing characters");
        return v;
    }
};

// decimal string (or JSON integer) -> 32 bytes little-endian
void put_int(const J& v, const std::string& what, std::vector<uint8_t>& out) {
    if ((v.kind != 's' && v.kind != 'n') || v.text.empty() || v.text.size() > 80) throw Bad{what + ": not a decimal integer"};
    uint8_t le[32];
    const cli::Decimal d = cli::parse_decimal(v.text.data(), v.text.size(), le);
    if (d != cli::Decimal::ok) throw Bad{what + (d == cli::Decimal::too_large ? ": above 2^256" : ": not a decimal integer")};
    out.insert(out.end(), le, le + 32);
}

const J& member(const J& o, const char* name, const std::string& what) {
    if (o.kind != 'o') throw Bad{what + ": not a JSON object"};
    auto it = o.members.find(name);
    if (it == o.members.end()) throw Bad{what + ": no \"" + name + "\""};
    return it->second;
}

bool is_one(const J& v) { return (v.kind == 's' || v.kind == 'n') && v.text == "1"; }
bool is_zero(const J& v) { return (v.kind == 's' || v.kind == 'n') && v.text == "0"; }

void put_g1(const J& p, const std::string& what, std::vector<uint8_t>& out) {
    if (p.kind != 'a' || p.items.size() != 3) throw Bad{what + ": a G1 point is [x, y, z]"};
    if (is_zero(p.items[2])) {
        out.insert(out.end(), 64, 0);
        return;
    }
    if (!is_one(p.items[2])) throw Bad{what + ": z must be \"1\" (affine) or \"0\" (infinity)"};
    put_int(p.items[0], what + ".x", out);
    put_int(p.items[1], what + ".y", out);
}

void put_g2(const J& p, const std::string& what, std::vector<uint8_t>& out) {
    auto pair = [&](const J& v, const char* c) {
        if (v.kind != 'a' || v.items.size() != 2) throw Bad{what + ": a G2 point is [[x0, x1], [y0, y1], [z0, z1]]"};
        (void)c;
    };
    if (p.kind != 'a' || p.items.size() != 3) throw Bad{what + ": a G2 point is [[x0, x1], [y0, y1], [z0, z1]]"};
    for (int k = 0; k < 3; ++k) pair(p.items[k], "");
    const J& z = p.items[2];
    if (is_zero(z.items[0]) && is_zero(z.items[1])) {
        out.insert(out.end(), 128, 0);
        return;
    }
    if (!is_one(z.items[0]) || !is_zero(z.items[1])) throw Bad{what + ": z must be [\"1\", \"0\"] (affine) or [\"0\", \"0\"] (infinity)"};
    put_int(p.items[0].items[0], what + ".x.c0", out);
    put_int(p.items[0].items[1], what + ".x.c1", out);
    put_int(p.items[1].items[0], what + ".y.c0", out);
    put_int(p.items[1].items[1], what + ".y.c1", out);
}

J read_json(const char* path) {
    std::vector<uint8_t> bytes;
    if (!cli::read_file(path, bytes)) throw Bad{std::string("cannot read ") + path};
    const std::string text(bytes.begin(), bytes.end());
    try {
        Parser p{text};
        return p.parse();
    } catch (const Bad& b) {
        throw Bad{std::string(path) + ": " + b.msg};
    }
}

const char* status_name(uint32_t s) {
    switch (s) {
        case GWB_G16V_PUBLIC: return "PUBLIC (a public signal is not below r)";
        case GWB_G16V_POINT: return "POINT (a coordinate is not below q, or a point is not on its curve)";
        case GWB_G16V_SUBGROUP: return "SUBGROUP (B is not in G2's order-r subgroup)";
        case GWB_G16V_EQUATION: return "EQUATION (the pairing equation does not hold)";
        default: return "unknown status";
    }
}

// "OK!", or the verdict and exit status 1; a failed call is exit status 2
int verdict(int rc, uint32_t status, gw_status_t& st, const char* point_refused) {
    if (rc != 0) return cli::report(2, st, "verify failed");
    if (status == GWB_G16V_VALID) {
        printf("OK!\n");
        return 0;
    }
    printf("INVALID: %s\n", status == GWB_G16V_POINT && point_refused ? point_refused : status_name(status));
    return 1;
}

// --compressed <vk.bin> <public.json> <proof.bin>
int verify_compressed(char** argv) {
    std::vector<uint8_t> key, pub, proof;
    for (int k = 0; k < 2; ++k)
        if (!cli::read_file(argv[k ? 4 : 2], k ? proof : key)) return cli::cannot_read(argv[k ? 4 : 2]);
    if (proof.size() != GWB_GROTH16_CPROOF_BYTES) {
        fprintf(stderr, "error: %s: %zu bytes, a compressed proof has %d\n", argv[4], proof.size(), GWB_GROTH16_CPROOF_BYTES);
        return 2;
    }
    gw_status_t st = {OK, NULL};
    gwb_g16vk_t* loaded = NULL;
    if (gwb_g16vk_load_compressed(key.data(), key.size(), &loaded, &st) != 0) return cli::fail(argv[2], st, "load failed");
    const Vk vk(loaded);
    gwb_g16vk_info_t info;
    gwb_g16vk_info(vk.get(), &info);
    try {
        const J pj = read_json(argv[3]);
        const std::string pv = argv[3];
        if (pj.kind != 'a') throw Bad{pv + ": public signals are not a list"};
        if (pj.items.size() != info.n_public)
            throw Bad{pv + ": " + std::to_string(pj.items.size()) + " public signals, the key has nPublic " + std::to_string(info.n_public)};
        for (size_t i = 0; i < pj.items.size(); ++i) put_int(pj.items[i], pv + ": signal " + std::to_string(i), pub);
    } catch (const Bad& b) {
        fprintf(stderr, "error: %s\n", b.msg.c_str());
        return 2;
    } catch (const std::exception& e) {
        fprintf(stderr, "error: %s\n", e.what());
        return 2;
    }
    uint32_t status = 0;
    const int rc = gwb_groth16_verify_batch_compressed_host(vk.get(), proof.data(), pub.data(), info.n_public, 1, &status, &st);
    return verdict(rc, status, st, "POINT (a point's compressed encoding is refused)");
}

}  // namespace

int main(int argc, char** argv) {
    if (argc == 5 && strcmp(argv[1], "--compressed") == 0) return verify_compressed(argv);
    if (argc != 4) {
        fprintf(stderr, "usage: %s <verification_key.json> <public.json> <proof.json>\n       %s --compressed <vk.bin> <public.json> <proof.bin>\n", argv[0],
                argv[0]);
        return 2;
    }
    std::vector<uint8_t> key, pub, proof;
    uint32_t n_public = 0;
    try {
        const J vk = read_json(argv[1]), pj = read_json(argv[2]), pr = read_json(argv[3]);
        const std::string kv = argv[1];
        const J& np = member(vk, "nPublic", kv);
        if (np.kind != 'n' || np.text.empty() || np.text.size() > 9 || np.text.find_first_not_of("0123456789") != std::string::npos)
            throw Bad{kv + ": nPublic is not a non-negative integer"};
        n_public = (uint32_t)std::stoul(np.text);
        const J& proto = member(vk, "protocol", kv);
        if (proto.kind != 's' || proto.text != "groth16") throw Bad{kv + ": protocol is not \"groth16\""};
        put_g1(member(vk, "vk_alpha_1", kv), kv + ": vk_alpha_1", key);
        put_g2(member(vk, "vk_beta_2", kv), kv + ": vk_beta_2", key);
        put_g2(member(vk, "vk_gamma_2", kv), kv + ": vk_gamma_2", key);
        put_g2(member(vk, "vk_delta_2", kv), kv + ": vk_delta_2", key);
        const J& ic = member(vk, "IC", kv);
        if (ic.kind != 'a') throw Bad{kv + ": IC is not a list"};
        for (size_t i = 0; i < ic.items.size(); ++i) put_g1(ic.items[i], kv + ": IC[" + std::to_string(i) + "]", key);
        const std::string pv = argv[2];
        if (pj.kind != 'a') throw Bad{pv + ": public signals are not a list"};
        if (pj.items.size() != n_public)
            throw Bad{pv + ": " + std::to_string(pj.items.size()) + " public signals, the key has nPublic " + std::to_string(n_public)};
        for (size_t i = 0; i < pj.items.size(); ++i) put_int(pj.items[i], pv + ": signal " + std::to_string(i), pub);
        const std::string rv = argv[3];
        put_g1(member(pr, "pi_a", rv), rv + ": pi_a", proof);
        put_g2(member(pr, "pi_b", rv), rv + ": pi_b", proof);
        put_g1(member(pr, "pi_c", rv), rv + ": pi_c", proof);
    } catch (const Bad& b) {
        fprintf(stderr, "error: %s\n", b.msg.c_str());
        return 2;
    } catch (const std::exception& e) {
        fprintf(stderr, "error: %s\n", e.what());
        return 2;
    }
    gw_status_t st = {OK, NULL};
    gwb_g16vk_t* loaded = NULL;
    if (gwb_g16vk_load(key.data(), key.size(), n_public, &loaded, &st) != 0) return cli::fail(argv[1], st, "load failed");
    const Vk vk(loaded);
    uint32_t status = 0;
    const int rc = gwb_groth16_verify_batch_host(vk.get(), proof.data(), pub.data(), n_public, 1, &status, &st);
    return verdict(rc, status, st, NULL);
}
