// Host build of the point codec (r1cs/point_codec_gfx950.hpp) for tests/test_point_codec_host.py (g++ -fsanitize=address,undefined):
// the section file of tests/native/point_codec.hip, record by record on the CPU through the same per-record function
// (point_codec_ops.hpp).  It holds no expected values.
//
//   point_codec_host IN OUT
//   IN  = sections { u32 op, n, in_words, out_words, param; u32 data[n * in_words] }
//   OUT = the sections' results back to back, (n + 64) * out_words u32 each: 64 guard records (0xa5 bytes) follow the results
#include <stdio.h>
#include <string.h>

#include <vector>

#include "point_codec_ops.hpp"

using namespace codec_ops;

template <uint32_t OP>
static void run(const uint32_t* in, uint32_t* out, uint32_t n) {
    for (uint32_t t = 0; t < n; ++t) run_record<OP>(in + (size_t)t * in_words(OP), out + (size_t)t * out_words(OP));
}

static bool dispatch(uint32_t op, const uint32_t* in, uint32_t* out, uint32_t n) {
    switch (op) {
#define CASE(OP) case OP: run<OP>(in, out, n); return true;
        CASE(OP_FQ_SQRT) CASE(OP_FQ2_SQRT) CASE(OP_FQ_IS_LARGER) CASE(OP_FQ2_IS_LARGER) CASE(OP_G1_ENCODE) CASE(OP_G2_ENCODE) CASE(OP_G1_DECODE)
        CASE(OP_G2_DECODE)
#undef CASE
    }
    return false;
}

int main(int argc, char** argv) {
    if (argc != 3) {
        fprintf(stderr, "usage: %s IN OUT\n", argv[0]);
        return 2;
    }
    FILE* f = fopen(argv[1], "rb");
    if (!f) {
        fprintf(stderr, "cannot read %s\n", argv[1]);
        return 2;
    }
    std::vector<uint32_t> file;
    {
        uint32_t buf[4096];
        size_t got;
        while ((got = fread(buf, 4, 4096, f)) > 0) file.insert(file.end(), buf, buf + got);
        fclose(f);
    }
    FILE* fo = fopen(argv[2], "wb");
    if (!fo) {
        fprintf(stderr, "cannot write %s\n", argv[2]);
        return 2;
    }
    size_t pos = 0;
    int sections = 0;
    while (pos < file.size()) {
        if (file.size() - pos < 5) {
            fprintf(stderr, "truncated section header\n");
            return 2;
        }
        const uint32_t op = file[pos], n = file[pos + 1], iw = file[pos + 2], ow = file[pos + 3];
        pos += 5;
        if (op < OP_FQ_SQRT || op >= OP_END || n == 0 || n > MAX_RECORDS || iw != in_words(op) || ow != out_words(op) ||
            (size_t)n * iw > file.size() - pos) {
            fprintf(stderr, "bad section (op %u, n %u, %u -> %u words)\n", op, n, iw, ow);
            return 2;
        }
        // the records in a buffer of their exact size, so that a read past the last one is seen
        const std::vector<uint32_t> in(file.begin() + pos, file.begin() + pos + (size_t)n * iw);
        std::vector<uint32_t> out((size_t)(n + GUARD) * ow, 0xa5a5a5a5u);
        if (!dispatch(op, in.data(), out.data(), n)) return 2;
        if (fwrite(out.data(), 4, out.size(), fo) != out.size()) {
            fprintf(stderr, "short write\n");
            return 2;
        }
        pos += (size_t)n * iw;
        ++sections;
    }
    fclose(fo);
    printf("point_codec_host: %d sections\n", sections);
    return 0;
}
