// The reference's symbol: gw_calc_witness (drop-in for reference src/lib.rs:44-111) -- one input set per call, the graph image
// with every call -- with its in-process handle cache and the on-disk program cache.
#include "runtime_internal.hpp"

namespace cwcrt {

// ---- compiled-graph cache for the single-shot entry point (the reference re-parses per call, lib.rs:129) ----
struct CacheEntry {
    uint64_t hash;
    std::vector<uint8_t> bytes;  // the graph image itself: a hit is a byte-for-byte match, never a hash alone
    std::shared_ptr<gwb_graph> g;
};
std::mutex g_cache_mu;
// (never destroyed: the handles own HIP objects and static destructors run after the HIP runtime may be gone)
std::vector<CacheEntry>& g_cache = *new std::vector<CacheEntry>();

// SHA-256 (FIPS 180-4) of the graph image: the key of the on-disk program cache
std::string sha256_hex(const uint8_t* p, size_t n) {
    static const uint32_t K[64] = {
        0x428a2f98, 0x71374491, 0xb5c0fbcf, 0xe9b5dba5, 0x3956c25b, 0x59f111f1, 0x923f82a4, 0xab1c5ed5, 0xd807aa98, 0x12835b01, 0x243185be, 0x550c7dc3, 0x72be5d74,
        0x80deb1fe, 0x9bdc06a7, 0xc19bf174, 0xe49b69c1, 0xefbe4786, 0x0fc19dc6, 0x240ca1cc, 0x2de92c6f, 0x4a7484aa, 0x5cb0a9dc, 0x76f988da, 0x983e5152, 0xa831c66d,
        0xb00327c8, 0xbf597fc7, 0xc6e00bf3, 0xd5a79147, 0x06ca6351, 0x14292967, 0x27b70a85, 0x2e1b2138, 0x4d2c6dfc, 0x53380d13, 0x650a7354, 0x766a0abb, 0x81c2c92e,
        0x92722c85, 0xa2bfe8a1, 0xa81a664b, 0xc24b8b70, 0xc76c51a3, 0xd192e819, 0xd6990624, 0xf40e3585, 0x106aa070, 0x19a4c116, 0x1e376c08, 0x2748774c, 0x34b0bcb5,
        0x391c0cb3, 0x4ed8aa4a, 0x5b9cca4f, 0x682e6ff3, 0x748f82ee, 0x78a5636f, 0x84c87814, 0x8cc70208, 0x90befffa, 0xa4506ceb, 0xbef9a3f7, 0xc67178f2};
    uint32_t h[8] = {0x6a09e667, 0xbb67ae85, 0x3c6ef372, 0xa54ff53a, 0x510e527f, 0x9b05688c, 0x1f83d9ab, 0x5be0cd19};
    auto rotr = [](uint32_t x, int k) { return (x >> k) | (x << (32 - k)); };
    auto block = [&](const uint8_t* b) {
        uint32_t w[64];
        for (int i = 0; i < 16; ++i) w[i] = ((uint32_t)b[4 * i] << 24) | ((uint32_t)b[4 * i + 1] << 16) | ((uint32_t)b[4 * i + 2] << 8) | b[4 * i + 3];
        for (int i = 16; i < 64; ++i) {
            const uint32_t s0 = rotr(w[i - 15], 7) ^ rotr(w[i - 15], 18) ^ (w[i - 15] >> 3), s1 = rotr(w[i - 2], 17) ^ rotr(w[i - 2], 19) ^ (w[i - 2] >> 10);
            w[i] = w[i - 16] + s0 + w[i - 7] + s1;
        }
        uint32_t a = h[0], bb = h[1], c = h[2], d = h[3], e = h[4], f = h[5], g = h[6], hh = h[7];
        for (int i = 0; i < 64; ++i) {
            const uint32_t S1 = rotr(e, 6) ^ rotr(e, 11) ^ rotr(e, 25), ch = (e & f) ^ (~e & g), t1 = hh + S1 + ch + K[i] + w[i];
            const uint32_t S0 = rotr(a, 2) ^ rotr(a, 13) ^ rotr(a, 22), mj = (a & bb) ^ (a & c) ^ (bb & c), t2 = S0 + mj;
            hh = g; g = f; f = e; e = d + t1; d = c; c = bb; bb = a; a = t1 + t2;
        }
        h[0] += a; h[1] += bb; h[2] += c; h[3] += d; h[4] += e; h[5] += f; h[6] += g; h[7] += hh;
    };
    size_t i = 0;
    for (; i + 64 <= n; i += 64) block(p + i);
    uint8_t tail[128] = {0};
    const size_t rem = n - i;
    memcpy(tail, p + i, rem);
    tail[rem] = 0x80;
    const size_t tl = rem + 9 <= 64 ? 64 : 128;
    const uint64_t bits = (uint64_t)n * 8;
    for (int k = 0; k < 8; ++k) tail[tl - 1 - k] = (uint8_t)(bits >> (8 * k));
    block(tail);
    if (tl == 128) block(tail + 64);
    char out[65];
    for (int k = 0; k < 8; ++k) snprintf(out + 8 * k, 9, "%08x", h[k]);
    return std::string(out, 64);
}

// On-disk cache of the single-shot entry point's compiled program: a process that has never seen a graph image finds the
// program an earlier process compiled for it (the first call otherwise parses, compiles and searches schedules).  One file
// per (SHA-256 of the image, library build): <dir>/<sha256>-<build>.cwcprog = the blob of gwb_graph_export (checksummed,
// structurally validated on import: a damaged or stale file is ignored and rewritten).  <dir> is Knobs::cache_dir: CWC_PROGRAM_CACHE=<dir>
// names it, CWC_PROGRAM_CACHE=0 turns the cache off; default $XDG_CACHE_HOME or ~/.cache, /circom-witnesscalc-amd.
std::string program_cache_file(const Knobs& k, const void* graph_data, size_t len) {
    if (k.cache_dir.empty()) return "";
    // (this build -- the content hash of every source under csrc/ as the Makefile stamped it, not a timestamp: the compiler
    // and the kernels that give a program its meaning are compiled separately from this file --, the program format, the
    // cost model's cycle table: a program is chosen under one table)
    static const std::string build = []() {
        const std::string id = std::string(CWC_TREE_HASH " format 18 table ") + std::to_string((unsigned long long)model_table_id());
        return sha256_hex((const uint8_t*)id.data(), id.size()).substr(0, 16);
    }();
    return k.cache_dir + "/" + sha256_hex((const uint8_t*)graph_data, len) + "-" + build + ".cwcprog";
}
// A cache file = 96 bytes that name what it is for -- "CWCPROG2", then <sha256 of the graph image>-<build> as in its file name,
// zero-padded -- followed by the blob of gwb_graph_export: a file that was renamed or copied over another entry, or written
// by another build under a colliding name, does not pass for this graph's program.
static const size_t kCacheHeader = 96;
std::string cache_entry_name(const std::string& path) {
    const size_t slash = path.rfind('/'), dot = path.rfind(".cwcprog");
    const size_t a = slash == std::string::npos ? 0 : slash + 1;
    return dot == std::string::npos || dot < a ? path.substr(a) : path.substr(a, dot - a);
}
std::vector<uint8_t> cache_wrap(const std::string& path, const void* blob, size_t n) {
    std::vector<uint8_t> out(kCacheHeader + n, 0);
    memcpy(out.data(), "CWCPROG2", 8);
    const std::string name = cache_entry_name(path);
    memcpy(out.data() + 8, name.data(), std::min(name.size(), kCacheHeader - 8));
    memcpy(out.data() + kCacheHeader, blob, n);
    return out;
}
bool cache_unwrap(const std::string& path, const std::vector<uint8_t>& file, const uint8_t** blob, size_t* n) {
    if (file.size() < kCacheHeader || memcmp(file.data(), "CWCPROG2", 8) != 0) return false;
    const std::string name = cache_entry_name(path);
    uint8_t want[kCacheHeader - 8] = {0};
    memcpy(want, name.data(), std::min(name.size(), sizeof want));
    if (name.size() > sizeof want || memcmp(file.data() + 8, want, sizeof want) != 0) return false;
    *blob = file.data() + kCacheHeader;
    *n = file.size() - kCacheHeader;
    return true;
}
bool read_file(const std::string& path, std::vector<uint8_t>& out) {
    FILE* f = fopen(path.c_str(), "rb");
    if (!f) return false;
    bool ok = fseek(f, 0, SEEK_END) == 0;
    const long n = ok ? ftell(f) : -1;
    ok = ok && n >= 0 && n < (1l << 31) && fseek(f, 0, SEEK_SET) == 0;
    if (ok) {
        out.resize((size_t)n);
        ok = fread(out.data(), 1, (size_t)n, f) == (size_t)n;
    }
    fclose(f);
    return ok;
}
void write_file_atomically(const std::string& path, const void* data, size_t n) {
    const size_t slash = path.rfind('/');
    if (slash != std::string::npos) {  // mkdir -p of the directory (two levels are enough for the default)
        const std::string dir = path.substr(0, slash);
        const size_t up = dir.rfind('/');
        if (up != std::string::npos && up > 0) (void)mkdir(dir.substr(0, up).c_str(), 0700);
        (void)mkdir(dir.c_str(), 0700);
    }
    const std::string tmp = path + ".tmp" + std::to_string((long)getpid());
    FILE* f = fopen(tmp.c_str(), "wb");
    if (!f) return;
    const bool ok = fwrite(data, 1, n, f) == n;
    if (fclose(f) != 0 || !ok || rename(tmp.c_str(), path.c_str()) != 0) (void)remove(tmp.c_str());
}

}  // namespace cwcrt

extern "C" {

// ---- the reference's symbol (src/lib.rs:44-111) ----------------------------------------------------
int gw_calc_witness(const char* inputs, const void* graph_data, const size_t graph_data_len, void** wtns_data,
                    size_t* wtns_len, const gw_status_t* status_c) {
    return guarded(const_cast<gw_status_t*>(status_c), [&]() -> int {
    gw_status_t* status = const_cast<gw_status_t*>(status_c);  // the reference writes through it too
    const Knobs k = read_knobs();
    if (!inputs) return fail(status, "inputs is null");                    // lib.rs:51-54
    if (!graph_data) return fail(status, "graph_data is null");            // lib.rs:56-59
    if (graph_data_len == 0) return fail(status, "graph_data_len is 0");   // lib.rs:61-64
    if (!wtns_data || !wtns_len) return fail(status, "wtns_data or wtns_len is null");
    // CStr::to_str UTF-8 check (lib.rs:72-84)
    {
        const unsigned char* s = (const unsigned char*)inputs;
        size_t i = 0, n = strlen(inputs);
        while (i < n) {
            unsigned char c = s[i];
            size_t k = c < 0x80 ? 1 : (c >> 5) == 6 ? 2 : (c >> 4) == 14 ? 3 : (c >> 3) == 30 ? 4 : 0;
            bool ok = k != 0 && i + k <= n;
            for (size_t q = 1; ok && q < k; ++q) ok = (s[i + q] & 0xC0) == 0x80;
            if (ok && k == 2) ok = c >= 0xC2;
            if (ok && k == 3) ok = !(c == 0xE0 && s[i + 1] < 0xA0) && !(c == 0xED && s[i + 1] >= 0xA0);
            if (ok && k == 4) ok = !(c == 0xF0 && s[i + 1] < 0x90) && !(c > 0xF4) && !(c == 0xF4 && s[i + 1] >= 0x90);
            if (!ok) return fail(status, "Failed to parse inputs: invalid utf-8 sequence at byte " + std::to_string(i));
            i += k;
        }
    }
    // calc_witness (lib.rs:125-136): inputs first, then the graph
    InputList list;
    std::string err;
    const bool dbg_single = k.debug_single;  // diagnostic: where a call's time goes
    auto now_ms = []() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
    const double t_in = now_ms();
    warm_device(k);
    if (!deserialize_inputs(inputs, strlen(inputs), list, err)) return fail(status, "Failed to calculate witness: " + err);
    const double t_inputs = now_ms();

    std::shared_ptr<gwb_graph> g;
    // (a sampled fingerprint picks the candidate, the byte compare below decides: hashing the whole 3 MB image on every
    // call was 2-3 ms of the single call's 12)
    const uint64_t h = sampled_fingerprint((const uint8_t*)graph_data, graph_data_len);
    {
        std::lock_guard<std::mutex> lk(g_cache_mu);
        for (auto& e : g_cache)
            if (e.hash == h && e.bytes.size() == graph_data_len && memcmp(e.bytes.data(), graph_data, graph_data_len) == 0) g = e.g;
    }
    if (!g) {
        const std::string cf = program_cache_file(k, graph_data, graph_data_len);  // (SHA-256 of the image: once per graph and process)
        std::vector<uint8_t> blob;
        if (!cf.empty() && read_file(cf, blob)) {  // a program an earlier process compiled for this very image (the import checks for a device behind its host work)
            gwb_graph_t* imported = nullptr;
            gw_status_t st2{OK, nullptr};
            const uint8_t* body = nullptr;
            size_t body_len = 0;
            if (!cache_unwrap(cf, blob, &body, &body_len)) set_status(&st2, ERROR, "not this graph's / this build's cache entry");
            else if (guarded(&st2, [&]() -> int { return import_graph(body, body_len, k, &imported, &st2); }) == 0) g.reset(imported);
            if (k.debug_cache) fprintf(stderr, "program cache: %s %s%s%s\n", g ? "hit" : "ignored", cf.c_str(), g ? "" : ": ", g ? "" : (st2.error_msg ? st2.error_msg : "?"));
            gwb_free_status(&st2);  // (a damaged / stale file: fall through to the compiler, the file is rewritten)
        }
        if (!g) {
            gwb_graph* raw = nullptr;
            if (load_graph(graph_data, graph_data_len, k, &raw, err)) return fail(status, "Failed to calculate witness: " + err);
            g.reset(raw);
            g->cache_path = cf;  // where the refined program goes once the background search has finished
        }
        std::lock_guard<std::mutex> lk(g_cache_mu);
        if (g_cache.size() >= 4) g_cache.erase(g_cache.begin());
        g_cache.push_back(CacheEntry{h, std::vector<uint8_t>((const uint8_t*)graph_data, (const uint8_t*)graph_data + graph_data_len), g});
    }
    std::vector<uint8_t> row((size_t)g->n_inputs * 32), wit((size_t)g->n_witness * 32);
    {
        Graph meta;  // populate_inputs only needs the input map (a handle imported from the cache holds no graph)
        meta.inputs = g->inputs;
        meta.input_index = g->input_index;
        if (!populate_inputs(list, meta, row.data(), g->n_inputs, err)) return fail(status, "Failed to calculate witness: " + err);
    }
    if (k.quirks)
        for (const auto& kv : list) {
            const InputSignal& s = g->inputs[g->input_index.at(kv.first)];
            printf("input %s, offset %u, len %u\n", kv.first.c_str(), s.offset, s.len);
        }
    uint32_t st = 0;
    const double t_graph = now_ms();
    double t_device = t_graph;
    {
        std::lock_guard<std::mutex> lk(g->mu);
        (void)pick_tile_width(g.get(), k, 1);  // host work first: a new graph's program is compiled while warm_device's thread brings the device up
        err = check_device();
        t_device = now_ms();
        if (err.empty()) err = run_host(g.get(), k, row.data(), 1, wit.data(), &st);
    }
    if (!err.empty()) return fail(status, "Failed to calculate witness: " + err);
    if (dbg_single) {
        gwb_timing_t tm;
        if (gwb_last_timing(g.get(), &tm) == 0)
            fprintf(stderr, "gw_calc_witness: program key %#x, %llu bundles, interpreter %.2f ms, pack %.2f ms | inputs %.1f ms, graph handle + input row %.1f ms, program choice + device check %.1f ms, upload + run %.1f ms\n",
                    g->last_key, (unsigned long long)tm.n_bundles, tm.interp_ms, tm.pack_ms, t_inputs - t_in, t_graph - t_inputs, t_device - t_graph, now_ms() - t_device);
    }
    // The program for the on-disk cache: the one the background search settled on (the quick first program is not worth
    // keeping).  Written by whichever call first finds the search finished.
    if (g->has_graph && !g->cache_written && !g->cache_path.empty()) {
        const std::string& cf = g->cache_path;
        uint32_t key = 0;
        {
            std::lock_guard<std::mutex> lk(g->mu);
            auto it = g->chosen.find(1);
            if (it != g->chosen.end() && !g->refining.count(1)) key = it->second;
        }
        if (!cf.empty() && key) {
            void* blob = nullptr;
            size_t blob_len = 0;
            gw_status_t st2{OK, nullptr};
            if (guarded(&st2, [&]() -> int { return export_graph(g.get(), k, key, &blob, &blob_len, &st2); }) == 0) {
                const std::vector<uint8_t> wrapped = cache_wrap(cf, blob, blob_len);
                write_file_atomically(cf, wrapped.data(), wrapped.size());
                if (k.debug_cache) fprintf(stderr, "program cache: wrote %s (program key %#x, %zu bytes)\n", cf.c_str(), key, blob_len);
            }
            gwb_free_status(&st2);
            free(blob);
            g->cache_written = true;
        }
    }
    if (st) return fail(status, "Failed to calculate witness: " + set_status_text(st));
    const size_t n = wtns_size(g->n_witness);
    void* buf = malloc(n);
    if (!buf) return fail(status, "Failed to allocate memory for wtns_data");  // lib.rs:99-102
    wtns_from_witness(wit.data(), g->n_witness, (uint8_t*)buf);
    *wtns_len = n;
    *wtns_data = buf;
    if (k.quirks) {
        set_status(status, ERROR, "test error");  // lib.rs:106
        printf("OK\n");                            // lib.rs:108
    } else {
        set_status(status, OK, "");
    }
    return 0;
    });
}

}  // extern "C"
