// The pack schedule of a program: the order in which its witness rows can be converted and stored while the interpreter
// is still running, derived from the program alone (hdr, recs, witness_refs) when it is uploaded.  Host only.
//
// Programs with one divider wave per interpreter wave and one stream (KEY_DIVIDER alone) give every tile a second
// wavefront that serves the division requests and is idle in between (kernels.hip, the `wave >= NW` branch).  That wave
// packs witness rows between requests: a row may be packed once the bundle that produces its slot has run AND its
// stores are known to have completed.  The interpreter issues a bundle's result stores one iteration late and waits for
// them with the counted wait at the top of its loop only (vmcnt(7): everything issued two iterations earlier has
// completed), so what the divider wave may rely on when it sees the post of request k is: every bundle in front of
// request k - 1 has its results in memory (requests are at least two bundles apart: REQ, GET, REQ).  The schedule counts
// readiness with that lag of one request.
#include "runtime_internal.hpp"

namespace cwcrt {

// Shader cycles of the replay below, MI355X.  The interpreter's bundles come from the cost model's class table
// (model_class_cycles); a request of up to 64 lanes is one safegcd inversion and one product on the divider wave
// (profiles/r03_inv_bench.txt: 52.2 k); a pack pass is 64 lanes = G entries x T sets loaded, converted and stored by the
// divider wave with the next pass's loads in flight: 2 188 cycles at T = 2, 2 304 at T = 4, the start of every gap included
// (stamped build, authV2-class graph, profiles/inline_pack_ab.txt).
static const double kCyclesDividerServe = 52200, kCyclesPackPass = 2300;

std::string make_pack_schedule(const Program& p, const Knobs& knobs, PackSchedule& out) {
    const uint32_t nw = p.n_witness, G = p.G, nreq = p.n_div_requests;
    out.order.resize(nw);
    out.ready.assign((size_t)nreq + 1, 0u);
    out.n_inline = 0;
    for (uint32_t i = 0; i < nw; ++i) out.order[i] = i;
    if (p.divider != 1 || p.n_streams != 1 || nreq == 0 || nw == 0 || G == 0) return "";  // out of scope: the pack kernel takes everything
    if (p.hdr.size() < p.n_bundles || p.recs.size() < (size_t)p.n_bundles * G * 4 || p.witness_refs.size() < nw) return "pack schedule: truncated program";
    // producer of a slot: the LAST bundle with a record whose destination is that slot (every record form stores to its
    // dst field: the four copies of a narrow product, the extra records of a fused node, both records of a scan pair,
    // collects, inputs; records without a result name the trash slot or nowhere)
    const uint64_t slot_bytes = 32ull * p.T, first_off = (uint64_t)p.n_const * slot_bytes, end_off = ((uint64_t)p.n_const + p.n_slots) * slot_bytes;
    const uint32_t kNever = 0xffffffffu;
    std::vector<uint32_t> producer(p.n_slots, kNever), req_bundle;
    req_bundle.reserve(nreq);
    for (uint32_t b = 0; b < p.n_bundles; ++b) {
        if ((p.hdr[b] & HDR_CLASS_MASK) == C_DIVREQ) req_bundle.push_back(b);
        for (uint32_t i = 0; i < G; ++i) {
            const uint64_t dst = p.recs[((size_t)b * G + i) * 4 + 2] & ~CTRL_MASK;
            if (dst >= first_off && dst < end_off) producer[(dst - first_off) / slot_bytes] = b;
        }
    }
    if (req_bundle.size() != nreq) return "pack schedule: the program has " + std::to_string(req_bundle.size()) + " request bundles, its header says " + std::to_string(nreq);
    // posts seen by the divider wave when entry w becomes packable: 0 for constants; a slot produced in front of request
    // k (0-based) is in memory when the post of request k + 1 is seen, that is with k + 2 posts
    std::vector<uint32_t> at(nw);
    for (uint32_t w = 0; w < nw; ++w) {
        const uint32_t ref = p.witness_refs[w];
        if (ref & REF_CONST) {
            at[w] = 0;
            continue;
        }
        const uint32_t slot = ref & ~REF_CANON;
        if (slot >= p.n_slots || producer[slot] == kNever) return "pack schedule: witness " + std::to_string(w) + " names a slot that no bundle writes";
        const uint32_t k = (uint32_t)(std::upper_bound(req_bundle.begin(), req_bundle.end(), producer[slot]) - req_bundle.begin());  // first request behind the producer
        at[w] = k + 2;  // (above nreq: never, the pack kernel's)
    }
    std::stable_sort(out.order.begin(), out.order.end(), [&](uint32_t a, uint32_t b) { return at[a] < at[b]; });  // (stable: by witness index inside one request)
    for (uint32_t w = 0; w < nw; ++w)
        if (at[w] <= nreq) out.ready[at[w]]++;
    for (uint32_t k = 1; k <= nreq; ++k) out.ready[k] += out.ready[k - 1];
    // Replay of a launch: how far the divider wave gets in the gaps between its requests.  In a gap it has seen k posts
    // (k requests served) and packs whole groups of G entries below ready[k]; a new post ends the gap.
    const double pass_cycles = knobs.pack_pass_cycles.value_or(kCyclesPackPass);  // (CWC_PACK_PASS_CYCLES: what-if runs, like CWC_MODEL_CYCLES)
    double clock = 0, div_free = 0, served = 0;
    uint32_t next = 0, k = 0;
    for (uint32_t b = 0; b < p.n_bundles && k <= nreq; ++b) {
        const uint32_t cls = p.hdr[b] & HDR_CLASS_MASK;
        clock += model_class_cycles((int)cls);
        if (cls == C_DIVREQ) {
            const uint32_t limit = std::min(out.ready[k], nw) / G * G;
            const double gap = clock - div_free;
            if (gap > 0 && limit > next) next += (uint32_t)std::min<double>(std::floor(gap / pass_cycles) * G, limit - next);
            served = std::max(clock, div_free) + kCyclesDividerServe;
            div_free = served;
            ++k;
        } else if (cls == C_DIVGET) {
            clock = std::max(clock, served);
        }
    }
    out.n_inline = std::min(next, out.ready[nreq]);
    return "";
}

}  // namespace cwcrt

static int schedule_out(const Program& p, const Knobs& k, uint32_t* pack_order, size_t order_cap, uint32_t* pack_ready, size_t ready_cap, uint32_t* n_witness, uint32_t* n_ready,
                        uint32_t* n_inline, gw_status_t* status) {
    PackSchedule s;
    const std::string err = make_pack_schedule(p, k, s);
    if (!err.empty()) return fail(status, err);
    if (n_witness) *n_witness = (uint32_t)s.order.size();
    if (n_ready) *n_ready = (uint32_t)s.ready.size();
    if (n_inline) *n_inline = s.n_inline;
    if (pack_order && order_cap >= s.order.size() && !s.order.empty()) memcpy(pack_order, s.order.data(), s.order.size() * 4);
    if (pack_ready && ready_cap >= s.ready.size()) memcpy(pack_ready, s.ready.data(), s.ready.size() * 4);
    set_status(status, OK, "");
    return 0;
}

extern "C" int gwb_pack_schedule_of_blob(const void* blob, size_t len, uint32_t* pack_order, size_t order_cap, uint32_t* pack_ready, size_t ready_cap,
                                         uint32_t* n_witness, uint32_t* n_ready, uint32_t* n_inline, gw_status_t* status) {
    return guarded(status, [&]() -> int {
        const Knobs k = read_knobs();
        if (!blob) return fail(status, "null argument");
        if (len < 24 + 8) return fail(status, "bad blob: too short");
        const uint8_t* b = (const uint8_t*)blob;
        uint64_t tr[3];  // (the trailer of gwb_graph_export: exact program length, padded length, checksum)
        memcpy(tr, b + len - 24, 24);
        if (tr[2] != blob_checksum(b, len - 24)) return fail(status, "bad blob: checksum mismatch (truncated or corrupted)");
        if (tr[0] > tr[1] || tr[1] > len - 24) return fail(status, "bad blob trailer");
        Program p;
        std::string err;
        if (!program_from_blob(b, (size_t)tr[0], p, err) || !validate_program(p, err)) return fail(status, "bad program blob: " + err);
        return schedule_out(p, k, pack_order, order_cap, pack_ready, ready_cap, n_witness, n_ready, n_inline, status);
    });
}

extern "C" int gwb_pack_schedule(gwb_graph_t* g, uint32_t program_key, uint32_t* pack_order, size_t order_cap, uint32_t* pack_ready, size_t ready_cap,
                                 uint32_t* n_witness, uint32_t* n_ready, uint32_t* n_inline, gw_status_t* status) {
    return guarded(status, [&]() -> int {
        const Knobs k = read_knobs();
        if (!g) return fail(status, "null argument");
        std::lock_guard<std::mutex> lk(g->mu);
        Program tmp;
        const Program* p = nullptr;
        if ((program_key & ~KEY_MODE_MASK) == 64) program_key = 64;
        auto it = g->progs.find(program_key);
        auto pre = g->compiled.find(program_key);
        std::string err;
        if (it != g->progs.end()) {
            p = &it->second->host;
        } else if (pre != g->compiled.end()) {
            p = pre->second.get();
        } else {
            if (!g->has_graph) return fail(status, "imported handle has no program for that key");
            if (!compile_program(g->graph, k, program_key & ~KEY_MODE_MASK, key_divider_waves(program_key), tmp, err, key_streams(program_key))) return fail(status, err);
            p = &tmp;
        }
        return schedule_out(*p, k, pack_order, order_cap, pack_ready, ready_cap, n_witness, n_ready, n_inline, status);
    });
}
