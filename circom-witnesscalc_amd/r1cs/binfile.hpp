// The section table of an iden3 binfile as the `.zkey` and `.ptau` loaders read it (zkey.cc, ptau.cc): four bytes of magic, u32
// version = 1, u32 nSections, then per section u32 id, u64 size, size bytes; sections in any order.  Hostile bytes in.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <string>
#include <vector>

namespace cwc_r1cs {

struct BinSection {
    const uint8_t* p = nullptr;  // into the caller's bytes; nullptr: the file has no such section
    uint64_t size = 0;
};

struct BinEntry {  // one section as the file has it, known id or not
    uint32_t id;
    const uint8_t* p;
    uint64_t size;
};

inline uint32_t rd32(const uint8_t* p) {
    uint32_t v;
    memcpy(&v, p, 4);
    return v;
}

// Walks the table of the file d[0 .. len) whose magic is `kind` ("zkey"), which also starts every message ("zkey: ...").  The
// sections whose id has its bit set in `accepted` (ids below 32) go to out[id], and none of them may occur twice; the others
// are passed over.  Every section must lie inside the file and the last one must end it.  order != nullptr gets every section
// in file order, the ones passed over included.
inline bool binfile_sections(const uint8_t* d, size_t len, const char* kind, uint32_t accepted, BinSection* out, std::string& err,
                             std::vector<BinEntry>* order = nullptr) {
    const std::string pre = std::string(kind) + ": ";
    if (len < 12 || memcmp(d, kind, 4) != 0) {
        err = pre + "bad magic (not a ." + kind + " file)";
        return false;
    }
    const uint32_t version = rd32(d + 4), n_sections = rd32(d + 8);
    if (version != 1) {
        err = pre + "unsupported version " + std::to_string(version) + " (1 expected)";
        return false;
    }
    uint64_t off = 12;
    for (uint32_t i = 0; i < n_sections; ++i) {
        if (len - off < 12) {
            err = pre + "truncated section header";
            return false;
        }
        const uint32_t id = rd32(d + off);
        uint64_t size;
        memcpy(&size, d + off + 4, 8);
        off += 12;
        if (size > len - off) {
            err = pre + "truncated section " + std::to_string(id) + " (declares " + std::to_string(size) + " bytes, " + std::to_string(len - off) +
                  " left)";
            return false;
        }
        if (id < 32 && ((accepted >> id) & 1u)) {
            if (out[id].p) {
                err = pre + "duplicate section " + std::to_string(id);
                return false;
            }
            out[id] = BinSection{d + off, size};
        }
        if (order) order->push_back(BinEntry{id, d + off, size});
        off += size;
    }
    if (off != len) {
        err = pre + std::to_string(len - off) + " trailing bytes after the last section";
        return false;
    }
    return true;
}

}  // namespace cwc_r1cs
