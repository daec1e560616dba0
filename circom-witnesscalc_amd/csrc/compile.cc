// Host graph compiler: the choice among schedule variants (compile_program) and the phases of one variant (compile_variant):
// validation, exact rewrites (power-of-two divisions, bit-extract fusion, tree-height reduction with shared subexpressions
// and dead-node elimination), node forms, the constant table, critical-path list scheduling into same-class bundles
// (schedule_program), operand routing (LDS ring vs. staged memory), liveness-based slot allocation and program encoding
// (format v4).  See program.hpp / program_dev.h.
#include <map>

#include "compile_internal.hpp"

namespace cwc {

// The rewritten graph (load-time optimiser, bit-extract fusion, tree-height reduction) depends on the fusion switch and on
// the weight table only: the schedule variants of one compile_program call share it instead of redoing it.
struct RewriteCache {
    struct Entry {
        bool bit_fusion;
        const uint32_t* table;  // kClassCost / kClassCostNarrow (before the linear-heavy switch and the A/B overrides)
        uint32_t G;             // (the tree-height reduction's leaf bound follows it)
        Graph g;
        ProgramStats st;
        const uint32_t* class_cost;
    };
    std::deque<Entry> entries;  // (a deque: entries stay where they are while other threads append)
    std::mutex* lock = nullptr; // set when the compiles of several threads share the cache
};
struct SharedRewrites {  // one cache and one lock per tile width 1, 2, .. 64: compiles of different widths do not wait for each other
    std::mutex m[7];
    RewriteCache cache[7];
};
SharedRewrites* make_shared_rewrites() {
    SharedRewrites* s = new SharedRewrites();
    for (int i = 0; i < 7; ++i) s->cache[i].lock = &s->m[i];
    return s;
}
void free_shared_rewrites(SharedRewrites* s) { delete s; }
static bool compile_variant(const Graph& g_in, uint32_t T, uint32_t divider, bool bit_fusion, const VariantOptions& opt, const Knobs& k, Program& out,
                            std::string& err, RewriteCache* cache = nullptr, bool probe_only = false, uint32_t streams = 1);

// Validation and statistics of a loaded graph without compiling a program (what gwb_graph_load needs).
bool probe_graph(const Graph& g, const Knobs& k, Program& out, std::string& err) {
    return compile_variant(g, 64, 0, false, VariantOptions{0, 0}, k, out, err, nullptr, true);
}

// The list scheduler is a heuristic, and exact rewrites and the narrow-bundle policy shift how the chains of a graph line
// up in bundles: the program is compiled with and without the bit-extract fusion, then under a few narrow-bundle
// policies, and the cheapest schedule by the measured cycles per bundle class (program_wave_cycles) is kept -- the
// policies are not fitted to one graph, the cost model picks per graph and tile width.
bool compile_program(const Graph& g, const Knobs& k, uint32_t T, uint32_t divider, Program& out, std::string& err, uint32_t streams, bool quick, SharedRewrites* shared) {
    const uint32_t G = T ? 64 / T : 1;
    VariantOptions base{k.coop_fill.value_or(G), k.coop_slack.value_or(~0u)};  // narrow whenever everything ready fits
    const bool forced = k.coop_fill || k.coop_slack;
    if (k.no_coop_mul || coop_nodes(T) == 0) base.fill = 0;
    RewriteCache own_cache;
    RewriteCache& cache = shared && T >= 1 && T <= 64 && !(T & (T - 1)) ? shared->cache[__builtin_ctz(T)] : own_cache;
    if (!compile_variant(g, T, divider, true, base, k, out, err, &cache, false, streams)) {
        // A fused form that cannot be scheduled must not fail the graph: the scan / convolution rewrites group nodes into one
        // bundle, and a grouping the detection should have rejected (a member that depends on another member) shows up as a
        // scheduler without ready nodes.  The program without convolution bundles, then without any scan chains, is always there.
        // (the scheduler's deadlock is named by ONE constant, kErrSchedulerDeadlock, here and where it is raised: rewording the message
        // cannot turn the fallback off; when every attempt fails the LAST attempt's error is what the caller sees)
        if (err != kErrSchedulerDeadlock) return false;
        base.no_conv = true;
        std::string err2;
        if (!compile_variant(g, T, divider, true, base, k, out, err2, &cache, false, streams)) {
            base.no_scans = true;
            if (!compile_variant(g, T, divider, true, base, k, out, err2, &cache, false, streams)) {
                err = err2;
                return false;
            }
        }
        err.clear();
    }
    if (quick || k.no_schedule_variants) return true;  // (quick: the first call on a graph runs this one schedule while the search runs in the background)
    // (one after the other: side by side on two threads the two compiles were no faster, 0.55 s either way for the
    // authV2-class graph, and slower for multi-million-node graphs)
    bool fusion = true;
    if (out.stats.n_bitx_nodes != 0 && !k.no_bit_fusion) {
        Program alt;
        std::string err2;
        if (compile_variant(g, T, divider, false, base, k, alt, err2, &cache, false, streams) && program_wave_cycles(alt) < program_wave_cycles(out)) {
            out = std::move(alt);
            fusion = false;
        }
    }
    // Representation inference is a heuristic too: where it had to insert conversions, the all-Montgomery program competes
    if (out.stats.n_conversions != 0 && !k.no_rep_inference && g.nodes.size() <= 2000000) {
        VariantOptions plain = base;
        plain.all_montgomery = true;
        Program alt;
        std::string err2;
        if (compile_variant(g, T, divider, fusion, plain, k, alt, err2, &cache, false, streams) && program_wave_cycles(alt) < program_wave_cycles(out)) {
            out = std::move(alt);
            base.all_montgomery = true;
        }
    }
    // Convolution bundles hold ONE limb product each: a long product (k = 32: 63 lanes busy for 32 rounds) always pays, many
    // small products that the unfused program runs side by side in a few full bundles may not -- the unfused program competes
    if (out.stats.n_conv_products != 0 && g.nodes.size() <= 2000000 && !k.conv_always) {
        VariantOptions plain = base;
        plain.no_conv = true;
        Program alt;
        std::string err2;
        if (compile_variant(g, T, divider, fusion, plain, k, alt, err2, &cache, false, streams) && program_wave_cycles(alt) < program_wave_cycles(out)) {
            out = std::move(alt);
            base.no_conv = true;
        }
    }
    if (base.fill == 0 || forced || g.nodes.size() > 2000000) return true;  // (huge graphs: one schedule, compile time counts)
    const VariantOptions more[] = {{0, 0}, {std::max(12u, G * 3 / 8), 0}, {G / 2, 2}, {G * 5 / 8, 2}};
    VariantOptions kept = base;
    for (VariantOptions pol : more) {
        pol.all_montgomery = base.all_montgomery;
        pol.no_conv = base.no_conv;
        pol.no_scans = base.no_scans;
        Program alt;
        std::string err2;
        if (compile_variant(g, T, divider, fusion, pol, k, alt, err2, &cache, false, streams) && program_wave_cycles(alt) < program_wave_cycles(out)) {
            out = std::move(alt);
            kept = pol;
        }
    }
    // Fused narrow chains (fuse_narrow_chains): how far from the critical path a chain is still fused is a policy too --
    // only the critical chain, chains within a few percent of it, every chain -- and the cost model picks
    // (CWC_FUSE=<thousandths + 1> forces one, CWC_NO_FUSE=1 none).
    if (T <= COOP_FUSE_MAX_T && kept.fill && !k.no_fuse) {
        std::vector<uint32_t> tries = {1, 11, 101, 1001, 0x10001, 0x1000b, 0x10065, 0x103e9};
        if (k.fuse) tries.assign(1, *k.fuse);
        for (uint32_t f : tries) {
            VariantOptions pol = kept;
            pol.fuse = f;
            Program alt;
            std::string err2;
            if (compile_variant(g, T, divider, fusion, pol, k, alt, err2, &cache, false, streams) && (k.fuse || program_wave_cycles(alt) < program_wave_cycles(out))) out = std::move(alt);
        }
    }
    return true;
}

// CWC_DEBUG_COMPILE_TIMES=1: seconds per phase on stderr
struct PhaseTimer {
    bool on;
    uint32_t T;
    std::chrono::steady_clock::time_point t = std::chrono::steady_clock::now();
    void start() { t = std::chrono::steady_clock::now(); }
    void operator()(const char* name) {
        if (!on) return;
        const auto now = std::chrono::steady_clock::now();
        fprintf(stderr, "compile T=%u: %-28s %.3f s\n", T, name, std::chrono::duration<double>(now - t).count());
        t = now;
    }
};

// ---- validate (assert_valid, reference src/graph.rs:343-356; evaluate() itself does not check) ----
static bool validate_operations(const Graph& g, const Graph& g_in, ProgramStats& st, std::string& err) {
    uint64_t arity_sum = 0;
    for (size_t i = 0; i < g.nodes.size(); ++i) {
        const Node& n = g.nodes[i];
        int ar = arity_of(n);
        if (n.kind == N_DUO && n.op == OP_POW) {  // graph.rs:141-142 unimplemented!
            err = "node " + std::to_string(i) + ": operator Pow not implemented for Montgomery";
            return false;
        }
        if (n.kind == N_UNO && n.op != UOP_NEG) {  // graph.rs:195
            err = "node " + std::to_string(i) + ": uno operator Id not implemented for Montgomery";
            return false;
        }
        if (ar) {
            st.n_op++;
            arity_sum += (uint64_t)ar + 1;
        } else if (n.kind == N_INPUT) {
            st.n_input_nodes++;
        }
    }
    for (uint32_t w : g_in.witness_signals)
        if (w >= g_in.nodes.size()) {
            err = "witness signal references node " + std::to_string(w) + " beyond the graph";
            return false;
        }
    st.algorithmic_bytes_per_set = 32ull * (arity_sum + 2 * st.n_input_nodes + 2 * st.n_witness);
    return true;
}

// ---- levels: the dependency depth, plain and with the steps of limb recurrences at a tenth of a level ----
static void compute_levels(const Graph& g, ProgramStats& st) {
    const size_t N = g.nodes.size();
    std::vector<uint32_t> level(N, 0);
    uint32_t depth = 0;
    for (size_t i = 0; i < N; ++i) {
        const Node& n = g.nodes[i];
        int ar = arity_of(n);
        if (!ar) continue;
        uint32_t l = level[n.a];
        if (ar >= 2) l = std::max(l, level[n.b]);
        if (ar >= 3) l = std::max(l, level[n.c]);
        level[i] = l + 1;
        depth = std::max(depth, l + 1);
    }
    st.depth = depth;
    // The same with the steps of limb recurrences -- an Idiv / Mod / Shr / Band of a sum, that sum, a product under it -- at a
    // tenth of a level: what the dependency depth comes to once such chains run as scan bundles (tile widths up to
    // SCAN_MAX_T; an estimate, used by the runtime to bound a program's size before anything is compiled).
    std::vector<uint8_t> step(N, 0);
    for (size_t i = N; i-- > 0;) {
        const Node& n = g.nodes[i];
        if (n.kind != N_DUO) continue;
        if ((n.op == OP_IDIV || n.op == OP_MOD || n.op == OP_SHR || n.op == OP_BAND) && g.nodes[n.a].kind == N_DUO && g.nodes[n.a].op == OP_ADD) step[i] = step[n.a] = 1;
        if (n.op == OP_ADD && step[i])
            for (uint32_t o : {n.a, n.b})
                if (g.nodes[o].kind == N_DUO && g.nodes[o].op == OP_MUL) step[o] = 1;
    }
    // (round 5) the one-bit recurrences of multi-register integers (rewrite.cc detect_bit_scans): a selection on an ordered comparison,
    // the comparison, and the short sums / differences under them (the arms x - y - bin, the comparand y + bin)
    {
        std::vector<uint8_t> reach(N, 0);  // how many more levels of Add / Sub below this node count as part of a step
        auto is_lin = [&](uint32_t o) { return g.nodes[o].kind == N_DUO && (g.nodes[o].op == OP_ADD || g.nodes[o].op == OP_SUB); };
        for (size_t i = N; i-- > 0;) {
            const Node& n = g.nodes[i];
            if (n.kind == N_TRES && g.nodes[n.a].kind == N_DUO && (g.nodes[n.a].op == OP_LT || g.nodes[n.a].op == OP_GT || g.nodes[n.a].op == OP_LEQ || g.nodes[n.a].op == OP_GEQ)) {
                step[i] = step[n.a] = 1;
                reach[n.a] = std::max<uint8_t>(reach[n.a], 1);
                for (uint32_t o : {n.b, n.c})
                    if (is_lin(o)) reach[o] = std::max<uint8_t>(reach[o], 3);
            }
            if (n.kind != N_DUO || !reach[i]) continue;
            if (is_lin((uint32_t)i)) step[i] = 1;
            for (uint32_t o : {n.a, n.b})
                if (is_lin(o)) reach[o] = std::max<uint8_t>(reach[o], (uint8_t)(is_lin((uint32_t)i) ? reach[i] - 1 : 1));
        }
    }
    std::vector<float> lf(N, 0.0f);
    float deepest = 0.0f;
    for (size_t i = 0; i < N; ++i) {
        const Node& n = g.nodes[i];
        const int ar = arity_of(n);
        if (!ar) continue;
        float l = lf[n.a];
        if (ar >= 2) l = std::max(l, lf[n.b]);
        if (ar >= 3) l = std::max(l, lf[n.c]);
        lf[i] = l + (step[i] ? 0.1f : 1.0f);
        deepest = std::max(deepest, lf[i]);
    }
    st.depth_scan = (uint64_t)deepest + 1;
}

// The working graph of a variant and the scheduling weights by class (class_cost may point at cost_override: the struct stays put).
struct PreparedGraph {
    Graph g;
    size_t n_in_buf = 0;
    const uint32_t* class_cost = nullptr;
    uint32_t cost_override[C_COUNT];
};

// ---- load-time re-optimiser, exact depth-reducing rewrites, scheduling weights ----
static void rewrite_graph(bool bit_fusion, uint32_t G, const uint32_t* weight_table, const Knobs& k, PhaseTimer& phase, ProgramStats& st, PreparedGraph& pg) {
    Graph& g = pg.g;
    // (the statistics above describe the graph as loaded)
    if (!k.no_load_optimize) {
        OptimizeStats os;
        if (k.random_eval) random_eval_passes(g, &os);
        optimize_loaded_graph(g, &os);
        st.n_folded = os.folded + os.random_constants;
        st.n_numbered = os.numbered + os.constants_merged + os.random_numbered;
        st.n_shaken = os.shaken;
        phase("load-time optimiser");
    }
    if (bit_fusion && !k.no_bit_fusion) {
        fuse_bit_extract(g);
        for (const Node& n : g.nodes) st.n_bitx_nodes += n.kind == N_DUO && n.op == OP_BITX;
        phase("bit-extract fusion");
    }
    // scheduling weights by class: linear-heavy graphs (more Add / Sub than Mul nodes) take the heavier linear weight
    pg.class_cost = weight_table;
    {
        size_t n_lin = 0, n_mul = 0;
        for (const Node& n : g.nodes) {
            n_lin += n.kind == N_DUO && (n.op == OP_ADD || n.op == OP_SUB);
            n_mul += n.kind == N_DUO && n.op == OP_MUL;
        }
        if (n_lin > n_mul && !k.no_lin_heavy_weights) pg.class_cost = kClassCostLinHeavy;
    }
    if (k.sched_lin_cost || k.sched_mul_cost) {  // (A/B knobs for the priority weights)
        for (int c = 0; c < (int)C_COUNT; ++c) pg.cost_override[c] = pg.class_cost[c];
        if (k.sched_lin_cost) pg.cost_override[C_LIN] = *k.sched_lin_cost;
        if (k.sched_mul_cost) pg.cost_override[C_MUL] = *k.sched_mul_cost;
        pg.class_cost = pg.cost_override;
    }
    if (G > 1 && !k.no_tree_reduction) {
        // whole chains at T = 1 (small batches: depth is everything); at most 8 leaves per tree otherwise, where the
        // extra nodes of wide trees cost lanes and memory traffic (measured on sha256_512: 293 k vs 265 k wit/s at 4096 sets)
        reduce_tree_height(g, k.tree_leaves.value_or(G >= 64 ? 64 : 8), pg.class_cost, k);  // (CWC_TREE_LEAVES: A/B knob)
    }
    for (const Node& n : g.nodes) st.n_op_compiled += arity_of(n) ? 1 : 0;
}

// Validate, levels, rewrites: the working graph (from the rewrite cache when a variant of the same call made it), its
// statistics and the scheduling weights.  probe_only: the graph as loaded, up to the levels.
static bool prepare_graph(const Graph& g_in, uint32_t T, uint32_t& divider, bool bit_fusion, const VariantOptions& opt, const Knobs& k, RewriteCache* cache,
                          bool probe_only, PhaseTimer& phase, Program& out, PreparedGraph& pg, std::string& err) {
    const uint32_t* weight_table = opt.fill && T <= 2 ? kClassCostNarrow : kClassCost;
    const RewriteCache::Entry* hit = nullptr;
    // (a shared cache: whoever comes first rewrites with the lock held, the others wait for the entry)
    std::unique_lock<std::mutex> cache_lock;
    if (cache && cache->lock) cache_lock = std::unique_lock<std::mutex>(*cache->lock);
    if (cache)
        for (const auto& e : cache->entries)
            if (e.bit_fusion == bit_fusion && e.table == weight_table && e.G == 64 / T) hit = &e;
    // validate operand order on the graph as loaded, then work on a rewritten copy
    for (size_t i = 0; !hit && i < g_in.nodes.size(); ++i) {
        const Node& n = g_in.nodes[i];
        const int ar = arity_of(n);
        if ((ar >= 1 && n.a >= i) || (ar >= 2 && n.b >= i) || (ar >= 3 && n.c >= i)) {
            err = "node " + std::to_string(i) + " references a node that is not before it";
            return false;
        }
        if (n.kind == N_CONST && n.a >= g_in.const_values.size()) {
            err = "node " + std::to_string(i) + ": bad constant index";
            return false;
        }
    }
    pg.g = hit ? hit->g : g_in;
    Graph& g = pg.g;
    if (hit && cache_lock.owns_lock()) cache_lock.unlock();
    phase.start();
    if (!hit) rewrite_pow2_divisions(g);
    const uint32_t G = 64 / T;
    if (divider != 0 && divider != 1 && divider != 3 && divider != 4) {
        err = "divider waves serve 1, 3 or 4 interpreter waves";
        return false;
    }
    if (G == 1) divider = 0;  // T = 64 keeps the reference's node order, one node per bundle
    out = Program();
    out.T = T;
    out.G = G;
    out.divider = divider;
    ProgramStats& st = out.stats;
    st.n_nodes = g_in.nodes.size();
    st.n_witness = g.witness_signals.size();
    pg.n_in_buf = inputs_buffer_size(g_in);
    // (the reference sizes the buffer from the leading Input nodes, lib.rs:138-152, and panics on anything beyond; here
    // the buffer covers every Input index and every signal of the input map -- within a sane bound: rows are n x 32 bytes)
    if (pg.n_in_buf > (1u << 27)) {
        err = "inputs buffer of " + std::to_string(pg.n_in_buf) + " elements is too large (an input map entry or Input index beyond 2^27)";
        return false;
    }
    if (hit) {
        st = hit->st;
        pg.class_cost = hit->class_cost;
        return true;
    }
    if (!validate_operations(g, g_in, st, err)) return false;
    phase("validate");
    compute_levels(g, st);
    phase("levels");
    if (probe_only) return true;
    rewrite_graph(bit_fusion, G, weight_table, k, phase, st, pg);
    if (cache && pg.class_cost != pg.cost_override) cache->entries.push_back(RewriteCache::Entry{bit_fusion, weight_table, G, g, st, pg.class_cost});
    return true;
}

// ---- one form per value (Montgomery or canonical, inserting the conversions; see infer_representations), scan chains
// (the steps of serial limb recurrences as pairs of N_SCAN nodes, class C_SCAN), fused narrow chains ----
static NodeForms choose_forms(Graph& g, uint32_t T, uint32_t divider, const VariantOptions& opt, const Knobs& k, const uint32_t* class_cost, PhaseTimer& phase,
                              ProgramStats& st) {
    const uint32_t G = 64 / T;
    NodeForms f;
    // (limb-arithmetic graphs -- the probe's scan-aware depth is well below the plain one -- at tile widths with the MODE 2 instances)
    // (The interpreter instances with scan / convolution / canonical-product paths, like the ones with fused narrow bundles, exist for
    // programs with no or one divider wave per interpreter: kernels.hip launch_interp.)
    const bool mode2_ok = T <= SCAN_MAX_T && G >= 2 && divider <= 1;
    const bool limb_graph = mode2_ok && !k.no_scan && st.depth_scan * 10 < st.depth * 8;
    // bit graphs (sha256-like: one operation in thirty-two or more is a bit extract): canonical inputs, every product canonical
    const bool bit_graph = mode2_ok && !k.no_bit_graph && !opt.all_montgomery && st.n_bitx_nodes * 32 >= st.n_op && st.n_op > 0;
    infer_representations(g, f.rep, f.vflags, st.n_conversions, st.n_canonical, opt.all_montgomery, (limb_graph || bit_graph) && !k.no_mul_cc, f.n_mul_cc, bit_graph, k);
    phase("representation inference");
    if (mode2_ok && !k.no_scan && !opt.no_scans) {
        detect_scans(g, f.rep, f.vflags, f.scan_imm, f.scan_partner, st.n_scan_steps, k);
        // borrow chains / most-significant-difference comparisons of multi-register integers (limb graphs: the step kinds live in the MODE 2 instances)
        if (limb_graph) detect_bit_scans(g, f.rep, f.vflags, f.scan_imm, f.scan_partner, st.n_scan_steps, k);
        // schoolbook limb products: the column sums of a k x k block as one bundle (2k - 1 columns, one node slot each)
        if (f.n_mul_cc && !opt.no_conv && !k.no_conv) detect_convolutions(g, f.rep, f.vflags, f.scan_imm, f.scan_partner, G, st.n_conv_products, k);
        phase("scan chains");
    }
    if (opt.fuse && opt.fill && T <= COOP_FUSE_MAX_T && G > 1 && divider <= 1 && st.n_scan_steps == 0 && f.n_mul_cc == 0) {  // (a program has fused bundles or scan bundles: one interpreter instance each)
        fuse_narrow_chains(g, f.rep, f.vflags, class_cost, (opt.fuse & 0xffffu) - 1, (opt.fuse & 0x10000u) != 0, st.n_fused_nodes);
        phase("fused narrow chains");
    }
    return f;
}

// ---- the floor of this execution model: the graph's longest dependent chain priced at the best measured latency of
// each operation on a lone wave, as pure arithmetic without any bundle's front end (bench.py roofline.chain) ----
static uint64_t chain_floor(const Graph& g) {
    // shader cycles: the four-lane product 704 (profiles/r03_ubench_coop_mul.txt), an addition 290, the safegcd inversion
    // 52 200 + its product (r03_inv_bench.txt), Fr::new of an input = one full-width product 1 436; integer classes at their
    // arithmetic on canonical operands; a round of a scan loop
    auto floor_cycles = [&](const Node& n) -> double {
        switch (class_of(n)) {
            case C_INPUT: return 1436;
            case C_MUL: return 704;
            case C_LIN: return 290;
            case C_DIV: return 52200 + 704;
            case C_CMPZ: return 100;
            case C_CMPS: return 400;
            case C_BIT: return 300;
            case C_IDIVMOD: return 1500;
            case C_TERN: return 100;
            case C_MULF: return 704.0 * (1 + (fused_op2(n.op) == FOP_MUL ? 1 : 0)) + 290.0 * ((fused_op2(n.op) > FOP_MUL ? 1 : 0) + (fused_op3(n.op) ? 1 : 0));
            case C_SCAN: return n.kind == N_CONV ? kCyclesConvStep * 32 : (n.op & SCAN_OP_DIV) ? kCyclesScanStepDiv : scan_is_sel(n.op) ? 150.0 : (n.op & (SCAN_OP_BORROW | SCAN_OP_LEX)) ? 20.0 : kCyclesScanStepCarry;  // (the serial rounds; chains of 64-bit limbs beat this "floor" with the parallel forms)
            default: return 0;
        }
    };
    const size_t N = g.nodes.size();
    std::vector<float> fin(N, 0.0f);
    double longest = 0;
    for (size_t i = 0; i < N; ++i) {
        const Node& n = g.nodes[i];
        if (n.kind == N_CONST) continue;
        const uint32_t ops[3] = {n.a, n.b, n.c};
        float t = 0;
        for (int q = 0; q < arity_of(n); ++q) t = std::max(t, fin[ops[q]]);
        fin[i] = t + (float)floor_cycles(n);
        longest = std::max(longest, (double)fin[i]);
    }
    return (uint64_t)longest;
}

// Operand q of node i, a constant: is it read in canonical form (the constant's canonical copy)?  Operands of integer-class
// nodes (shift amounts, masks, divisors, bounds) and of additions / selections / equality tests of canonical values are.
static bool reads_canonical_constants(const Graph& g, const NodeForms& f, size_t i, int q) {
    const Node& n = g.nodes[i];
    const int c = class_of(n);
    if (is_integer_class(c)) return q < 2 && !(n.op == OP_BITX && q == 1);
    if (c == C_CMPZ) return (n.op == OP_EQ || n.op == OP_NEQ) && (f.vflags[i] & VF_A_CANON);
    if (c == C_LIN) return f.rep[i] == REP_C;
    if (c == C_MULF) {  // the operand of an addition stage follows the node's form; a factor of a product is a Montgomery constant
        const bool lin_operand = fused_sq(n.op) ? (q == 1 ? fused_op2(n.op) > FOP_MUL : q == 2) : (q == 2 && fused_op2(n.op) > FOP_MUL);
        return lin_operand && f.rep[i] == REP_C;
    }
    if (c == C_TERN) return q >= 1 && f.rep[i] == REP_C;
    if (c == C_SCAN && n.kind == N_SCAN && scan_is_sel(n.op))  // a selection moves words: its arms in the form of its value, a comparison's operands canonical, a condition either way
        return (n.op & SCAN_OP_ACC) ? f.rep[i] == REP_C : true;
    if (c == C_SCAN) return true;  // x, the accumulator, the divisor: canonical integers
    if (c == C_MUL) return (f.vflags[i] & VF_MUL_CC) != 0;  // canonical products (bit graphs: with a constant's canonical copy)
    return false;  // Mul / Div: Montgomery form
}

struct ConstTable {
    std::vector<uint32_t> ref;  // for consts: REF_CONST|idx ; for others: slot (filled by the encoder)
    std::unordered_map<uint32_t, uint32_t> canon_const;  // constant node -> table index of its canonical copy
    uint32_t zero_const;  // index of the trailing dummy (value 0)
};

// ---- constants -> table (Montgomery form, then the canonical copies that are read), node -> ref ----
static ConstTable build_constant_table(const Graph& g, const NodeForms& f, Program& out) {
    const size_t N = g.nodes.size();
    ConstTable ct;
    ct.ref.assign(N, 0);
    for (size_t i = 0; i < N; ++i)
        if (g.nodes[i].kind == N_CONST) {
            Fr m = fr_to_mont(g.const_values[g.nodes[i].a]);
            ct.ref[i] = REF_CONST | (uint32_t)(out.consts.size() / 8);
            out.consts.insert(out.consts.end(), m.v, m.v + 8);
        }
    out.stats.n_const = out.consts.size() / 8;
    for (size_t i = 0; i < N; ++i) {
        const Node& n = g.nodes[i];
        const uint32_t ops[3] = {n.a, n.b, n.c};
        for (int q = 0; q < arity_of(n); ++q) {
            const uint32_t o = ops[q];
            if (g.nodes[o].kind != N_CONST || ct.canon_const.count(o) || !reads_canonical_constants(g, f, i, q)) continue;
            ct.canon_const[o] = (uint32_t)(out.consts.size() / 8);
            const Fr& v = g.const_values[g.nodes[o].a];
            out.consts.insert(out.consts.end(), v.v, v.v + 8);
        }
    }
    ct.zero_const = (uint32_t)(out.consts.size() / 8);
    out.consts.insert(out.consts.end(), 8, 0u);  // trailing dummy entry: the table is never empty (prefetch target)
    out.n_const = (uint32_t)(out.consts.size() / 8);
    return ct;
}

// diagnostic (CWC_DEBUG_NODE_MIX): what the scheduled graph is made of -- per (class, operation): nodes, and how their operands were produced
static void dump_node_mix(const Graph& g, uint32_t T) {
    std::map<std::string, uint64_t> mix;
    static const char* kOps[] = {"Mul", "Div", "Add", "Sub", "Pow", "Idiv", "Mod", "Eq", "Neq", "Lt", "Gt", "Leq", "Geq", "Land", "Lor", "Shl", "Shr", "Bor", "Band", "Bxor", "BitX"};
    auto name_of = [&](const Node& n) -> std::string {
        switch (n.kind) {
            case N_CONST: return "const";
            case N_INPUT: return "input";
            case N_UNO: return "Neg";
            case N_TRES: return "Tern";
            case N_FUSED: return "fused";
            case N_CONV: return "conv";
            case N_SCAN: return std::string(scan_is_sel(n.op) ? "sel" : (n.op & SCAN_OP_LEX) ? "lex" : (n.op & SCAN_OP_BORROW) ? "borrow" : (n.op & SCAN_OP_DIV) ? "sdiv" : "carry") + ((n.op & SCAN_OP_ACC) ? ".acc" : ".out");
            default: return n.op < sizeof kOps / sizeof *kOps ? kOps[n.op] : "?";
        }
    };
    for (const Node& n : g.nodes) {
        if (n.kind == N_CONST) continue;
        std::string key = name_of(n) + "(";
        const uint32_t ops[3] = {n.a, n.b, n.c};
        for (int q = 0; q < arity_of(n); ++q) key += (q ? ", " : "") + name_of(g.nodes[ops[q]]);
        mix[key + ")"]++;
    }
    std::vector<std::pair<uint64_t, std::string>> v;
    for (auto& kv : mix) v.push_back({kv.second, kv.first});
    std::sort(v.rbegin(), v.rend());
    fprintf(stderr, "node mix of the scheduled graph (T = %u):\n", T);
    for (size_t k = 0; k < v.size() && k < 60; ++k) fprintf(stderr, "  %8llu  %s\n", (unsigned long long)v[k].first, v[k].second.c_str());
}

// ---- the scheduler (schedule_program): the order of evaluated nodes (inputs + ops) and the bundle boundaries, per stream.
// G == 1: file order (the reference's own loop order; best locality, every bundle is one node anyway).
// G  > 1: list scheduling.  One bundle = up to G ready nodes of ONE class; a node is ready when all its
// producers sit in earlier bundles.  The class of the next bundle is that of the ready node with the longest
// cost-weighted path to a sink (critical path first); nodes with slack wait until their class comes up, so
// chains that are at different op classes in the same dependency level share bundles across levels instead
// of costing one bundle per (level, class).
// Streams: the graph's independent parts (components that share nothing but Input nodes and constants) can be
// evaluated by different wavefronts of one tile, each with its own bundle sequence.  Stream 0 also evaluates every
// Input node first (the prologue) and then posts; the other streams begin with a wait for that post.

namespace {

static const uint64_t kPrologueBoost = 1ull << 60;
static const uint32_t kConvKey = 1u << 20;  // the heap of convolution groups (a group is named by its column-0 node)

// G == 1: one node per bundle in file order
void schedule_file_order(const Graph& g, Schedule& sc) {
    for (size_t i = 0; i < g.nodes.size(); ++i)
        if (g.nodes[i].kind != N_CONST) {
            sc.bundle_of[i] = sc.use_bundle_of[i] = (uint32_t)sc.bundle_start.size();
            sc.bundle_start.push_back((uint32_t)sc.order.size());
            sc.bundle_coop.push_back(0);
            sc.bundle_flags.push_back(0);
            sc.order.push_back((uint32_t)i);
            sc.order_pos.push_back(0);
        }
    sc.s_count[0] = (uint32_t)sc.bundle_start.size();
}

struct Priorities {
    std::vector<std::vector<uint32_t>> users;  // adjacency (only non-const producers)
    std::vector<uint64_t> height;              // cost-weighted path to a sink
    std::vector<uint16_t> dist_to_div;         // operations between a node and the nearest division that depends on it (saturating)
    // Programs of several streams: the prologue -- Input nodes and the operations within a short chain of them, which
    // the graph's parts tend to share (flags, key bits, common subexpressions) -- is evaluated by stream 0 before
    // anything else; it posts behind it, the other streams begin with a wait for that post.
    std::vector<uint8_t> prologue;
};

// diagnostic (CWC_DEBUG_CRITICAL_PATH): class composition of the cost-weighted critical path
void dump_critical_path(const Graph& g, const Priorities& pr) {
    const size_t N = g.nodes.size();
    uint32_t cur = 0xffffffffu;
    for (size_t i = 0; i < N; ++i)
        if (g.nodes[i].kind != N_CONST && (cur == 0xffffffffu || pr.height[i] > pr.height[cur])) cur = (uint32_t)i;
    uint64_t cnt[C_COUNT] = {0}, total = pr.height[cur];
    std::string seq;
    while (true) {
        const int c = std::max(0, class_of(g.nodes[cur]));
        cnt[c]++;
        if (seq.size() < 400) seq += "IMLD?????T"[c < 10 ? c : 4];
        uint32_t nxt = 0xffffffffu;
        for (uint32_t u : pr.users[cur])
            if (nxt == 0xffffffffu || pr.height[u] > pr.height[nxt]) nxt = u;
        if (nxt == 0xffffffffu) break;
        cur = nxt;
    }
    fprintf(stderr, "critical path: cost %llu; nodes by class:", (unsigned long long)total);
    for (int c = 0; c < (int)C_COUNT; ++c)
        if (cnt[c]) fprintf(stderr, " %d:%llu", c, (unsigned long long)cnt[c]);
    fprintf(stderr, "\n  start: %s\n", seq.c_str());
}

void compute_priorities(const Graph& g, const NodeForms& f, const uint32_t* class_cost, const Knobs& k, Priorities& pr) {
    const size_t N = g.nodes.size();
    pr.height.assign(N, 0);
    pr.users.resize(N);
    for (size_t i = 0; i < N; ++i) {
        const Node& n = g.nodes[i];
        const uint32_t ops[3] = {n.a, n.b, n.c};
        uint32_t seen[3];
        int ns = 0;
        for (int q = 0; q < arity_of(n); ++q) {
            const uint32_t o = ops[q];
            if (g.nodes[o].kind == N_CONST) continue;
            bool dup = false;
            for (int z = 0; z < ns; ++z) dup |= seen[z] == o;
            if (dup) continue;
            seen[ns++] = o;
            pr.users[o].push_back((uint32_t)i);
        }
    }
    // (a selection step's ACC value depends on the operands of its OUT node -- the condition, the comparison's operands -- though it does not
    // name them: the OUT node is as urgent as the ACC node, or whatever computes the condition would be scheduled as if nothing waited for it)
    std::vector<uint64_t>& height = pr.height;
    const bool any_sel = !f.scan_partner.empty();
    for (size_t i = N; i-- > 0;) {
        if (g.nodes[i].kind == N_CONST) continue;
        uint64_t h = 0;
        for (uint32_t u : pr.users[i]) h = std::max(h, height[u]);
        const bool sel = any_sel && g.nodes[i].kind == N_SCAN && scan_is_sel(g.nodes[i].op);
        if (sel && !(g.nodes[i].op & SCAN_OP_ACC)) h = std::max(h, height[i]);  // (OUT in front of its ACC node: pre-set below)
        height[i] = h + node_cost(class_cost, g.nodes[i]);
        if (sel && (g.nodes[i].op & SCAN_OP_ACC)) {
            const uint32_t o = f.scan_partner[i];
            if (o > i) {  // the OUT node was visited already (a plain selection's: behind the graph's last node); its operands come later
                height[o] = std::max(height[o], height[i]);
            } else {
                height[o] = std::max(height[o], h);  // picked up when the loop reaches it
            }
        }
    }
    if (k.debug_critical_path) dump_critical_path(g, pr);
    static const uint32_t kFar = 0xffffu;
    pr.dist_to_div.assign(N, (uint16_t)kFar);
    for (size_t i = N; i-- > 0;) {
        if (g.nodes[i].kind == N_CONST) continue;
        if (class_of(g.nodes[i]) == C_DIV) {
            pr.dist_to_div[i] = 0;
            continue;
        }
        uint32_t d = kFar;
        for (uint32_t u : pr.users[i]) d = std::min<uint32_t>(d, pr.dist_to_div[u] + 1u);
        pr.dist_to_div[i] = (uint16_t)std::min<uint32_t>(d, kFar);
    }
    pr.prologue.assign(N, 0);
}

// Scan chains: a step is scheduled as a unit (its OUT node stands for both), consecutive steps of a chain go into
// consecutive pairs of ONE bundle.  A bundle's steps share kind and shift: one ready heap per (kind, shift).
struct ScanGroups {
    bool any = false;
    std::unordered_map<uint32_t, std::vector<uint32_t>> conv_members;  // column-0 node -> the group's nodes in column order
    std::vector<uint32_t> keys;  // distinct (kind << 8 | shift)
    std::vector<uint32_t> next;  // ACC node -> OUT node of the step that continues its chain
    int key_index(uint32_t key) const {
        for (size_t k = 0; k < keys.size(); ++k)
            if (keys[k] == key) return (int)k;
        return -1;
    }
    int heap_of(uint32_t key) const { return (int)C_SCAN + (int)C_COUNT * (17 + key_index(key)); }  // (scan steps: heap C_SCAN + C_COUNT * (17 + key index))
};
uint32_t scan_key_of(const Graph& g, const NodeForms& f, uint32_t i) { return (scan_kind_bits(g.nodes[i].op) << 8) | scan_shift_of(g, f, i); }  // (kind bits 0x02 .. 0xf0, a shift below 254)

void find_scan_groups(const Graph& g, const NodeForms& f, const ProgramStats& st, ScanGroups& sg) {
    sg.any = st.n_scan_steps != 0 || st.n_conv_products != 0;
    if (!sg.any) return;
    const size_t N = g.nodes.size();
    sg.next.assign(N, 0xffffffffu);
    for (size_t i = 0; i < N; ++i) {
        const Node& n = g.nodes[i];
        if (n.kind == N_CONV) {
            if (sg.key_index(kConvKey) < 0) sg.keys.push_back(kConvKey);
            std::vector<uint32_t>& m = sg.conv_members[f.scan_partner[i]];
            if (m.empty()) m.assign(2 * (f.scan_imm[i] >> 8) - 1, 0xffffffffu);
            m[f.scan_imm[i] & 0xffu] = (uint32_t)i;
            continue;
        }
        if (n.kind != N_SCAN || (n.op & SCAN_OP_ACC)) continue;
        const uint32_t key = scan_key_of(g, f, (uint32_t)i);
        if (sg.key_index(key) < 0) sg.keys.push_back(key);
        const Node& pr = g.nodes[n.b];
        if (!(n.op & SCAN_OP_NOACC) && !scan_is_sel(n.op) && pr.kind == N_SCAN && (pr.op & SCAN_OP_ACC) && scan_key_of(g, f, n.b) == key && sg.next[n.b] == 0xffffffffu) sg.next[n.b] = (uint32_t)i;  // (a selection stands alone)
    }
}

// what every stream's list scheduler works with
struct ListParams {
    uint32_t T, G, divider;
    // Narrow multiplication bundles: when no more multiplications are ready than four-lane products fit a wave, the
    // bundle is compiled for the lane-cooperative multiplier (about half the cycles of a full-width multiplication
    // bundle).
    size_t coop_cap, coop_fill;
    uint64_t coop_slack;
    const Knobs& k;
};

// diagnostic (CWC_DEBUG_SCHED): the first bundles, node by node
void dump_bundle(const Graph& g, const Priorities& pr, uint32_t b, int cl, const std::vector<uint32_t>& nodes) {
    fprintf(stderr, "bundle %u class %d:", b, cl);
    for (size_t q = 0; q < nodes.size() && q < 6; ++q) {
        const Node& dn = g.nodes[nodes[q]];
        fprintf(stderr, " [%u k%d op%d (%u,%u,%u) h%llu]", nodes[q], dn.kind, dn.op, dn.a, dn.b, dn.c, (unsigned long long)pr.height[nodes[q]]);
    }
    fprintf(stderr, "%s\n", nodes.size() > 6 ? " ..." : "");
}

// One stream's bundle sequence (bundle indices relative to the stream's first bundle) and the list scheduler that makes it.
// Producers in another stream do not gate a node (the streams' phases do).
struct StreamSched {
    std::vector<uint32_t> order, bundle_start, div_lanes;
    std::vector<uint32_t> order_pos;     // record position of every entry of `order` inside its bundle
    std::vector<uint8_t> bundle_coop;    // 0 full-width, 1 narrow multiplication bundle, 2 fused narrow bundle
    std::vector<uint32_t> bundle_flags;  // HDR_POST / HDR_WAIT: the bundle is a C_SYNC bundle
    uint32_t n_div_requests = 0;

    const Graph& g; const NodeForms& f; const Priorities& pr; const ScanGroups& sg; const ListParams& lp;
    Schedule& sc;  // (bundle_of / use_bundle_of: relative to the stream's first bundle until it is appended)
    const uint32_t s;

    // ready heaps per class, keyed by (height, ~index) so that ties prefer file order
    // (integer-class nodes: one heap per combination of operand / result forms, a bundle's header bits are uniform)
    typedef std::pair<uint64_t, uint32_t> Key;
    std::vector<std::vector<Key>> heap;
    std::vector<uint32_t> indeg;
    size_t remaining = 0, prologue_left = 0;
    std::vector<uint8_t> placed;      // scan nodes that sit in a bundle already (a step's successor inside its own bundle is released with it)
    std::vector<uint8_t> sel_queued;  // selection steps that sit in their ready heap
    std::unordered_map<uint32_t, uint32_t> conv_ready;  // group -> how many of its nodes have their operands
    // Asynchronous divider: a division bundle is split into a request (operands to the divider wave) and, about
    // one inversion later on the scheduler's clock, a collect bundle with the same nodes in the same node slots;
    // the interpreter runs other ready work in between.  One request is in flight at a time.
    uint64_t clock = 0;
    std::vector<uint32_t> in_flight;  // nodes of the pending request
    uint64_t in_flight_ready = 0;

    StreamSched(const Graph& g, const NodeForms& f, const Priorities& pr, const ScanGroups& sg, const ListParams& lp, Schedule& sc, uint32_t s)
        : g(g), f(f), pr(pr), sg(sg), lp(lp), sc(sc), s(s) {}
    uint32_t tie(uint32_t x) const { return lp.k.sched_tie_reverse ? x : ~x; }  // node <-> the second half of its Key
    void push_key(int hc, uint64_t h, uint32_t i) {
        auto& hs = heap[hc];
        hs.push_back(Key(h + (pr.prologue[i] ? kPrologueBoost : 0ull), tie(i)));
        std::push_heap(hs.begin(), hs.end());
    }
    uint32_t pop(std::vector<Key>& h) {
        std::pop_heap(h.begin(), h.end());
        const uint32_t i = tie(h.back().second);
        h.pop_back();
        return i;
    }
    // the non-empty heap with the most urgent top among those `ok` admits (-1: none)
    template <class Ok> int most_urgent(Ok ok) const {
        int best = -1;
        for (int c = 0; c < (int)heap.size(); ++c)
            if (!heap[c].empty() && ok(c) && (best < 0 || heap[c].front() > heap[best].front())) best = c;
        return best;
    }
    bool is_scan_heap(int c) const { return c % (int)C_COUNT == (int)C_SCAN && c >= (int)C_COUNT * 17; }

    void push(uint32_t i);
    void emit_bundle(const std::vector<uint32_t>& nodes, bool request, bool collect, int coop = 0, uint32_t sync_flags = 0);
    int choose_heap() const;
    void take_scan_bundle(int best, std::vector<uint32_t>& picked);
    void take_bundle(int best, std::vector<uint32_t>& picked);
    bool run(bool several, std::string& err);
    void number_positions();
};

void StreamSched::push(uint32_t i) {
    int hc = class_of(g.nodes[i]);
    if (hc == C_SCAN && g.nodes[i].kind == N_CONV) {  // a group goes into ONE bundle, once the last of its factors is there
        const uint32_t head = f.scan_partner[i];
        const std::vector<uint32_t>& m = sg.conv_members.find(head)->second;
        if (++conv_ready[head] < m.size()) return;
        uint64_t hgt = 0;
        for (uint32_t u : m) hgt = std::max(hgt, pr.height[u]);
        push_key(sg.heap_of(kConvKey), hgt, head);
        return;
    }
    if (hc == C_SCAN && scan_is_sel(g.nodes[i].op)) {  // a selection's two nodes name different operands: ready when both are
        const uint32_t o = (g.nodes[i].op & SCAN_OP_ACC) ? f.scan_partner[i] : i;
        if (placed[o] || sel_queued[o] || indeg[o] != 0 || indeg[f.scan_partner[o]] != 0) return;
        sel_queued[o] = 1;
        push_key(sg.heap_of(scan_key_of(g, f, o)), std::max(pr.height[o], pr.height[f.scan_partner[o]]), o);
        return;
    }
    if (hc == C_SCAN) {  // the step's OUT node stands for the pair
        if ((g.nodes[i].op & SCAN_OP_ACC) || placed[i]) return;
        push_key(sg.heap_of(scan_key_of(g, f, i)), std::max(pr.height[i], pr.height[f.scan_partner[i]]), i);
        return;
    }
    const uint8_t vf = f.vflags[i];
    if (hc == C_MUL && (vf & VF_MUL_CC)) hc += (int)C_COUNT;  // (canonical products: bundles of their own, never narrow)
    else if (hc == C_BIT) hc += (int)C_COUNT * (1 + vf + 8 * (g.nodes[i].op == OP_SHR || g.nodes[i].op == OP_BAND ? 1 : 0));  // (bundles of Shr / Band nodes take a straight path)
    else if (is_integer_class(hc)) hc += (int)C_COUNT * (1 + vf);
    else if (hc == C_CMPZ) hc += (int)C_COUNT * (1 + (vf & VF_OUT_CANON));
    else if (hc == C_MULF) {  // fused nodes: one heap per combination of stages (a bundle runs every stage one of its nodes has)
        const uint8_t op = g.nodes[i].op;
        hc += (int)C_COUNT * (1 + ((fused_op2(op) == FOP_MUL ? 1 : 0) | (fused_op2(op) > FOP_MUL ? 2 : 0) | (fused_op3(op) ? 4 : 0)));
    }
    push_key(hc, pr.height[i], i);
}

// coop: 0 full-width, 1 narrow multiplication bundle (C_MULQ), 2 fused narrow bundle (C_MULF)
void StreamSched::emit_bundle(const std::vector<uint32_t>& nodes, bool request, bool collect, int coop, uint32_t sync_flags) {
    const uint32_t b = (uint32_t)bundle_start.size();
    bundle_start.push_back((uint32_t)order.size());
    bundle_coop.push_back((uint8_t)coop);
    bundle_flags.push_back(sync_flags);
    if (b < lp.k.debug_sched) {
        const int cl = sync_flags ? (int)C_SYNC : request ? (int)C_DIVREQ : collect && lp.divider ? (int)C_DIVGET : coop == 2 ? (int)C_MULF : coop ? (int)C_MULQ : nodes.empty() ? (int)C_LIN : class_of(g.nodes[nodes[0]]);
        dump_bundle(g, pr, b, cl, nodes);
    }
    for (uint32_t i : nodes) {
        if (pr.prologue[i] && !request) --prologue_left;
        if (request) {
            sc.use_bundle_of[i] = b;
            order.push_back(i | REQ_FLAG);
        } else {
            sc.bundle_of[i] = b;
            if (!collect) sc.use_bundle_of[i] = b;
            order.push_back(i);
        }
    }
    if (request) return;
    remaining -= nodes.size();
    for (uint32_t i : nodes)  // release users only now: a bundle never reads its own results (but for the steps of a scan bundle: push skips them)
        for (uint32_t u : pr.users[i])
            if (sc.stream_of[u] == s && --indeg[u] == 0) push(u);
}

// the heap the next bundle comes from (-1: nothing is ready)
int StreamSched::choose_heap() const {
    int best = most_urgent([](int) { return true; });
    if (!in_flight.empty() && best == C_DIV)  // a second request has to wait for the first one: run the best other class
        best = most_urgent([](int c) { return c != C_DIV; });
    if (best < 0) return best;
    // An inversion bundle costs about thirty multiplication bundles however few of its lanes are used, and a
    // wave's time is the sum of its bundles: a ready division waits while another chain is within a few
    // operations of its own division (its ready node goes first), so that sibling chains divide together.
    if (best == C_DIV) {
        // the heap top is the class's most urgent node; scan the ready nodes of the class for one that
        // is about to reach a division
        const int other = most_urgent([&](int c) {
            if (c == C_DIV) return false;
            bool near = false;
            for (const Key& k : heap[c]) near |= pr.dist_to_div[tie(k.second)] <= lp.k.sched_div_wait;
            return near;
        });
        if (other >= 0) best = other;
    }
    // A scan bundle costs its front end however few steps it runs, and a wave's time is the sum of its bundles: while the
    // chain of the most urgent ready step goes on with steps whose other operands are not computed yet, anything else
    // that is ready runs first (it has to run anyway), so that chains go into few, full bundles.
    const int conv_heap = sg.key_index(kConvKey) < 0 ? -1 : sg.heap_of(kConvKey);
    if (is_scan_heap(best) && best != conv_heap && !lp.k.scan_eager) {
        const uint32_t head = tie(heap[best].front().second);
        size_t len_ready = 1, len_all = 1;
        bool contiguous = true;
        for (uint32_t cur = head; len_all < lp.G / 2; ++len_all) {
            const uint32_t nx = sg.next[f.scan_partner[cur]];
            if (nx == 0xffffffffu || sc.stream_of[nx] != s || placed[nx]) break;
            contiguous = contiguous && indeg[nx] == 1 && indeg[f.scan_partner[nx]] == 1;  // (one producer left: the accumulator; users[] holds a user once per producer)
            len_ready += contiguous;
            cur = nx;
        }
        if (len_ready < len_all) {
            const int other = most_urgent([&](int c) { return c % (int)C_COUNT != (int)C_SCAN && !(c == C_DIV && !in_flight.empty()); });
            if (other >= 0) best = other;
        }
    }
    // INPUT nodes first whenever any is ready (they have no producers and feed everything)
    if (!heap[C_INPUT].empty()) best = C_INPUT;
    return best;
}

// the most urgent ready step and, pair after pair, the steps that continue its chain -- as far as every other
// operand of theirs was produced by an earlier bundle --, then the next ready chain of the same kind
void StreamSched::take_scan_bundle(int best, std::vector<uint32_t>& picked) {
    auto& h = heap[best];
    const size_t cap_steps = lp.G / 2;
    auto in_bundle = [&](uint32_t x) { return std::find(picked.begin(), picked.end(), x) != picked.end(); };
    uint32_t longest = 0;
    while (picked.size() / 2 < cap_steps && !h.empty()) {
        uint32_t cur = pop(h);
        uint32_t run = 0;
        for (;;) {
            picked.push_back(cur);
            picked.push_back(f.scan_partner[cur]);
            placed[cur] = placed[f.scan_partner[cur]] = 1;
            ++run;
            if (picked.size() / 2 >= cap_steps) break;
            const uint32_t nx = sg.next[f.scan_partner[cur]];
            if (nx == 0xffffffffu || sc.stream_of[nx] != s || placed[nx]) break;
            const Node& nn = g.nodes[nx];
            if (indeg[nx] != 1 || indeg[f.scan_partner[nx]] != 1) break;
            if ((!(nn.op & SCAN_OP_NOX) && in_bundle(nn.a)) || (scan_has_third(nn.op) && in_bundle(nn.c))) break;  // (x or the divisor / subtrahend / comparand comes out of this very bundle)
            cur = nx;
        }
        longest = std::max(longest, run);
    }
    emit_bundle(picked, false, false);
    clock += 14 + (uint64_t)longest * scan_cost50(g.nodes[picked[0]].op);
}

// a bundle of the class of heap `best` (any class but the scan steps')
void StreamSched::take_bundle(int best, std::vector<uint32_t>& picked) {
    const uint32_t T = lp.T, G = lp.G;
    auto& h = heap[best];
    // a request must fit the interpreter's mailbox (mbox_lanes active lanes = node slots x T)
    const bool fused = best >= (int)C_COUNT && best % (int)C_COUNT == (int)C_MULF;  // fused narrow bundle: at most coop_nodes(T) nodes
    const size_t cap = best == C_DIV && lp.divider ? std::max<size_t>(1, std::min<size_t>(G, mbox_lanes(lp.divider) / T)) : fused ? (size_t)coop_nodes(T) : G;
    bool coop = false;
    if (best == C_MUL && lp.coop_cap) {
        // Narrow or full-width?  The ready multiplications in priority order; the ones within `coop_slack` of the
        // most urgent node's height cannot wait.  If they fit a narrow bundle it is one (cheapest step for the
        // critical chain; its free groups take the next most urgent multiplications, then linear riders) and the
        // rest stays ready: work with slack piles up until it becomes urgent itself and then fills full-width
        // bundles properly (a full-width bundle costs the same with 10 or 32 nodes).
        std::vector<Key> cand;
        while (!h.empty() && cand.size() < G) {
            std::pop_heap(h.begin(), h.end());
            cand.push_back(h.back());
            h.pop_back();
        }
        const uint64_t slack = lp.coop_slack;
        size_t n_urgent = 0;
        while (n_urgent < cand.size() && (slack >= cand[0].first || cand[n_urgent].first >= cand[0].first - slack)) ++n_urgent;
        coop = n_urgent <= lp.coop_cap && (cand.size() <= lp.coop_cap || cand.size() < lp.coop_fill);
        const size_t take = coop ? std::min(lp.coop_cap, cand.size()) : cand.size();
        for (size_t q = 0; q < cand.size(); ++q) {
            if (q < take) {
                picked.push_back(tie(cand[q].second));
            } else {
                h.push_back(cand[q]);
                std::push_heap(h.begin(), h.end());
            }
        }
    }
    while (!coop && !h.empty() && picked.size() < cap) picked.push_back(pop(h));
    std::sort(picked.begin(), picked.end());
    // the free node slots of a bundle take ready nodes of heap `from`, most urgent first, up to `limit` (sorted, behind the rest)
    auto fill_from = [&](std::vector<Key>& from, size_t limit) {
        std::vector<uint32_t> extra;
        while (!from.empty() && picked.size() + extra.size() < limit) extra.push_back(pop(from));
        std::sort(extra.begin(), extra.end());
        picked.insert(picked.end(), extra.begin(), extra.end());
    };
    if (fused && picked.size() < cap && !heap[C_MUL].empty()) fill_from(heap[C_MUL], cap);  // free groups of a fused bundle take ready plain multiplications
    // A wave's time is the sum of its bundles and a multiplication bundle costs the same however few of its
    // node slots are used: ready Add/Sub nodes ride in its free slots (the kernel then also runs the ~40-slot
    // linear body, header bits) instead of asking for a bundle of their own later.
    const size_t slots = coop ? lp.coop_cap : G;  // (a narrow bundle takes riders too: groups of four lanes add / subtract)
    if (best == C_MUL && picked.size() < slots && !heap[C_LIN].empty() && !lp.k.no_ride_along) fill_from(heap[C_LIN], slots);  // (multiplications first: they name the class)
    if (best == C_DIV && lp.divider) {
        emit_bundle(picked, true, false);
        in_flight = picked;
        clock += kClockCost[C_DIVREQ];
        in_flight_ready = clock + div_cost50();
    } else {
        emit_bundle(picked, false, false, fused ? 2 : coop ? 1 : 0);
        clock += cost_of(kClockCost, coop ? (int)C_MULQ : best % (int)C_COUNT);
    }
}

bool StreamSched::run(bool several, std::string& err) {
    const size_t N = g.nodes.size();
    const std::vector<uint8_t>& so = sc.stream_of;
    indeg.assign(N, 0);
    bool posted = !(several && s == 0);  // stream 0 of several: a post bundle right behind the last prologue node
    for (size_t i = 0; i < N; ++i) {
        if (g.nodes[i].kind == N_CONST) continue;
        for (uint32_t u : pr.users[i])
            if (so[u] == s && so[i] == s) indeg[u]++;
        remaining += so[i] == s;
        prologue_left += so[i] == s && pr.prologue[i];
    }
    heap.resize((size_t)C_COUNT * (17 + sg.keys.size()));
    if (sg.any) placed.assign(N, 0);
    if (sg.any) sel_queued.assign(N, 0);
    for (size_t i = 0; i < N; ++i)
        if (g.nodes[i].kind != N_CONST && so[i] == s && indeg[i] == 0) push((uint32_t)i);
    std::vector<uint32_t> picked;
    if (s != 0) {  // the wait for stream 0's post (the prologue's values), then two idle bundles: the staging loads of
                   // bundles 0 and 1 are issued before the loop and those of bundle 2 in front of the wait
        emit_bundle(picked, false, false, 0, HDR_WAIT);
        emit_bundle(picked, false, false);
        emit_bundle(picked, false, false);
    }
    const int conv_heap = sg.key_index(kConvKey) < 0 ? -1 : sg.heap_of(kConvKey);
    while (remaining) {
        if (!posted && prologue_left == 0 && in_flight.empty()) {  // (the post's vmcnt(0) covers every store issued so far)
            emit_bundle(std::vector<uint32_t>(), false, false, 0, HDR_POST);
            posted = true;
            continue;
        }
        // collect when the quotients are due, or when nothing else can run (the interpreter then waits)
        if (!in_flight.empty() && (clock >= in_flight_ready || most_urgent([](int c) { return c != C_DIV; }) < 0)) {
            emit_bundle(in_flight, false, true);
            div_lanes.push_back((uint32_t)in_flight.size() * lp.T);
            in_flight.clear();
            n_div_requests++;
            clock += kClockCost[C_DIVGET];
            continue;
        }
        const int best = choose_heap();
        if (best < 0) {
            err = kErrSchedulerDeadlock;
            return false;
        }
        picked.clear();
        if (best == conv_heap) {  // the columns of one limb product, position c = column c
            picked = sg.conv_members.find(pop(heap[best]))->second;
            emit_bundle(picked, false, false);
            clock += 14 + 70;
        } else if (is_scan_heap(best)) {
            take_scan_bundle(best, picked);
        } else {
            take_bundle(best, picked);
        }
    }
    if (!posted) emit_bundle(std::vector<uint32_t>(), false, false, 0, HDR_POST);
    number_positions();
    return true;
}

// record positions: a bundle's nodes sit at positions 0, 1, .. in the order the scheduler picked them
void StreamSched::number_positions() {
    const uint32_t nb = (uint32_t)bundle_start.size();
    order_pos.resize(order.size());
    for (uint32_t b = 0; b < nb; ++b) {
        const uint32_t e = b + 1 < nb ? bundle_start[b + 1] : (uint32_t)order.size();
        for (uint32_t k = bundle_start[b]; k < e; ++k) order_pos[k] = k - bundle_start[b];
    }
}

// diagnostic (CWC_DEBUG_STREAMS): the largest components and their streams
template <class Comp> void dump_streams(uint32_t T, const std::vector<Comp>& comps, const std::vector<uint32_t>& by_size, const std::vector<uint8_t>& comp_stream) {
    fprintf(stderr, "streams T=%u: %zu components;", T, comps.size());
    for (size_t q = 0; q < by_size.size() && q < 10; ++q) {
        const Comp& co = comps[by_size[q]];
        fprintf(stderr, " [%llu nodes, chain %.2f M, work %.2f M -> %u]", (unsigned long long)co.nodes, co.cp / 1e6, co.work / 1e6, comp_stream[by_size[q]]);
    }
    fprintf(stderr, "\n");
}

// ---- partition into streams: the prologue (pr.prologue), then the components of the rest, longest first, each to the
// stream with the least load so far (sc.stream_of, sc.P, sc.s_chain) ----
bool partition_streams(const Graph& g, const NodeForms& f, const ListParams& lp, uint32_t streams, bool refuse_one_part, Priorities& pr, Schedule& sc, std::string& err) {
    const size_t N = g.nodes.size();
    const uint32_t divider = lp.divider;
    std::vector<uint8_t>& prologue = pr.prologue;
    // components of the operation nodes (edges through Input nodes and constants do not connect)
    std::vector<uint32_t> parent(N);
    for (size_t i = 0; i < N; ++i) parent[i] = (uint32_t)i;
    auto find = [&](uint32_t x) {
        while (parent[x] != x) x = parent[x] = parent[parent[x]];
        return x;
    };
    auto unite = [&](uint32_t a, uint32_t b) {
        const uint32_t ra = find(a), rb = find(b);
        if (ra != rb) parent[ra] = rb;
    };
    auto is_op = [&](uint32_t i) { return arity_of(g.nodes[i]) != 0; };
    // per component: the longest dependent chain and the summed work, both in lone-wave cycles (a multiplication
    // on a chain is a narrow bundle where the tile width has them; a division is its request, the inversion and
    // its collect bundle)
    const bool narrow = lp.coop_cap != 0;
    auto node_cycles = [&](int c) -> double {
        if (c == C_MUL) return narrow ? kCycles[C_MULQ] : kCycles[C_MUL];
        if (c == C_MULF) return kCycles[C_MULF];
        if (c == C_SCAN) return 0.5 * (kCyclesScanStepCarry + kCyclesScanStepDiv);  // (a step's round of the loop)
        if (c == C_DIV && divider) return kCycles[C_DIV] + kCycles[C_DIVREQ] + kCycles[C_DIVGET];
        return kCycles[c];
    };
    const double theta = lp.k.stream_prologue;
    std::vector<double> cp(N, 0);
    for (size_t i = 0; i < N; ++i) {
        const Node& n = g.nodes[i];
        if (n.kind == N_INPUT) prologue[i] = 1;
        if (!is_op((uint32_t)i)) continue;
        const uint32_t ops[3] = {n.a, n.b, n.c};
        double m = 0;
        for (int q = 0; q < arity_of(n); ++q) m = std::max(m, cp[ops[q]]);
        cp[i] = m + node_cycles(class_of(n));
        prologue[i] = cp[i] <= theta;
        // (a selection step's two nodes name different operands and sit in one bundle: the later one brings both to the longer chain --
        // one of them in the prologue and the other in a stream of its own would tear the bundle apart)
        if (n.kind == N_SCAN && scan_is_sel(n.op)) {
            const uint32_t o = f.scan_partner[i];
            if (n.op & SCAN_OP_ACC) {
                // the ACC node decides for both: ITS users come behind it in node order and take their chain from it, so it must know
                // the condition's chain now -- the OUT node's operands all precede this node (they were the selection's, or its
                // comparison's, operands), whether the OUT node itself sits in front of it or behind the graph's last node
                const Node& on = g.nodes[o];
                const uint32_t oops[3] = {on.a, on.b, on.c};
                double mo = 0;
                for (int q = 0; q < arity_of(on); ++q) mo = std::max(mo, cp[oops[q]]);
                cp[i] = std::max(cp[i], mo + node_cycles(class_of(n)));
                prologue[i] = cp[i] <= theta;
                if (o < i) {
                    cp[o] = cp[i];
                    prologue[o] = prologue[i];
                }
            } else if (o < i) {  // (an OUT node behind its ACC node)
                cp[i] = cp[o];
                prologue[i] = prologue[o];
            }
        }
    }
    for (size_t i = 0; i < N; ++i) {
        if (!is_op((uint32_t)i) || prologue[i]) continue;
        const Node& n = g.nodes[i];
        const uint32_t ops[3] = {n.a, n.b, n.c};
        for (int q = 0; q < arity_of(n); ++q)
            if (is_op(ops[q]) && !prologue[ops[q]]) unite((uint32_t)i, ops[q]);
        if (n.kind == N_SCAN || n.kind == N_CONV) unite((uint32_t)i, f.scan_partner[i]);  // the two nodes of a step / the columns of a product sit in one bundle: one part (their operands may all be prologue values)
    }
    struct Comp { uint32_t root; double cp = 0, work = 0, alone = 0; uint64_t nodes = 0; };
    std::unordered_map<uint32_t, uint32_t> comp_index;
    std::vector<Comp> comps;
    for (size_t i = 0; i < N; ++i) {
        if (!is_op((uint32_t)i) || prologue[i]) continue;
        const Node& n = g.nodes[i];
        const int c = class_of(n);
        const uint32_t r = find((uint32_t)i);
        auto it = comp_index.find(r);
        if (it == comp_index.end()) {
            it = comp_index.emplace(r, (uint32_t)comps.size()).first;
            comps.push_back(Comp());
            comps.back().root = r;
        }
        Comp& co = comps[it->second];
        co.cp = std::max(co.cp, cp[i]);
        const double cap = ((c == C_MUL && narrow) || c == C_MULF) ? (double)std::max<size_t>(1, lp.coop_cap) : c == C_DIV && divider ? std::max(1.0, (double)mbox_lanes(divider) / lp.T) : (double)lp.G;
        co.work += node_cycles(c) / cap;
        co.nodes++;
    }
    for (Comp& co : comps) co.alone = std::max(co.cp, co.work);
    std::vector<uint32_t> by_size(comps.size());
    for (size_t k = 0; k < comps.size(); ++k) by_size[k] = (uint32_t)k;
    std::sort(by_size.begin(), by_size.end(), [&](uint32_t x, uint32_t y) { return comps[x].alone > comps[y].alone; });
    // longest first, each to the stream with the least load so far
    std::vector<uint8_t> comp_stream(comps.size(), 0);
    double load[MAX_STREAMS] = {0, 0, 0, 0};
    for (uint32_t k : by_size) {
        uint32_t to = 0;
        for (uint32_t s = 1; s < streams; ++s)
            if (load[s] < load[to]) to = s;
        comp_stream[k] = (uint8_t)to;
        load[to] += comps[k].alone;
    }
    uint32_t used = 0;
    for (uint32_t s = 0; s < streams; ++s) used += load[s] > 0;
    if (lp.k.debug_streams) dump_streams(lp.T, comps, by_size, comp_stream);
    if (used > 1) {
        sc.P = streams;  // (a stream without a part stays empty: its wave ends at once)
        for (size_t i = 0; i < N; ++i)
            if (is_op((uint32_t)i) && !prologue[i]) {
                sc.stream_of[i] = comp_stream[comp_index[find((uint32_t)i)]];
                sc.s_chain[sc.stream_of[i]] = std::max(sc.s_chain[sc.stream_of[i]], cp[i]);
            }
    } else {
        // one part only: the program would be the one-stream program of the same key.  Among the candidates of a
        // choice (shared rewrites) that sibling is being compiled anyway: refuse, the caller drops this key
        // (10.5 M nodes: half of the choice's compile work).
        if (refuse_one_part) {
            err = "the graph has one independent part: a stream program would equal the one-stream program";
            return false;
        }
        std::fill(prologue.begin(), prologue.end(), 0);
    }
    return true;
}

// stream s's bundles behind those of the streams before it
void append_stream(const Graph& g, uint32_t divider, uint32_t s, const StreamSched& ss, Schedule& sc) {
    const uint32_t nb = (uint32_t)ss.bundle_start.size();
    const uint32_t base = (uint32_t)sc.bundle_start.size();
    sc.s_first[s] = base;
    sc.s_count[s] = nb;
    sc.s_div[s] = ss.n_div_requests;
    const uint32_t obase = (uint32_t)sc.order.size();
    for (uint32_t b = 0; b < nb; ++b) {
        sc.bundle_start.push_back(obase + ss.bundle_start[b]);
        sc.bundle_coop.push_back(ss.bundle_coop[b]);
        sc.bundle_flags.push_back(ss.bundle_flags[b]);
    }
    for (uint32_t e : ss.order) {
        const uint32_t i = e & ~REQ_FLAG;
        if (e & REQ_FLAG) {
            sc.use_bundle_of[i] += base;
        } else {
            sc.bundle_of[i] += base;
            if (!(divider && class_of(g.nodes[i]) == C_DIV)) sc.use_bundle_of[i] += base;
        }
    }
    sc.order.insert(sc.order.end(), ss.order.begin(), ss.order.end());
    sc.order_pos.insert(sc.order_pos.end(), ss.order_pos.begin(), ss.order_pos.end());
    sc.div_lanes.insert(sc.div_lanes.end(), ss.div_lanes.begin(), ss.div_lanes.end());
    sc.n_div_requests += ss.n_div_requests;
}

}  // namespace

bool schedule_program(const Graph& g, const NodeForms& f, const ProgramStats& st, const uint32_t* class_cost, const VariantOptions& opt, const Knobs& k,
                      uint32_t T, uint32_t divider, uint32_t streams, bool refuse_one_part, Schedule& sc, std::string& err) {
    const size_t N = g.nodes.size();
    const uint32_t G = 64 / T;
    sc.order.reserve(N);
    sc.bundle_of.assign(N, 0xffffffffu);
    sc.use_bundle_of.assign(N, 0xffffffffu);
    sc.stream_of.assign(N, 0);
    if (G == 1) {
        schedule_file_order(g, sc);
    } else {
        Priorities pr;
        compute_priorities(g, f, class_cost, k, pr);
        ScanGroups sg;
        find_scan_groups(g, f, st, sg);
        const ListParams lp{T, G, divider, opt.fill ? coop_nodes(T) : 0, opt.fill, opt.slack_levels == ~0u ? ~0ull : (uint64_t)opt.slack_levels * class_cost[C_MUL], k};
        if (streams > 1 && (divider == 0 || divider == 1) && !partition_streams(g, f, lp, streams, refuse_one_part, pr, sc, err)) return false;
        // ---- schedule every stream; a stream's first bundle index is a multiple of the pipeline depths ----
        for (uint32_t s = 0; s < sc.P; ++s) {
            bool any = s == 0;
            for (size_t i = 0; i < N && !any; ++i) any = g.nodes[i].kind != N_CONST && sc.stream_of[i] == s;
            if (!any) {
                sc.s_first[s] = (uint32_t)sc.bundle_start.size();
                continue;
            }
            StreamSched ss(g, f, pr, sg, lp, sc, s);
            if (!ss.run(sc.P > 1, err)) return false;
            append_stream(g, divider, s, ss, sc);
            while (s + 1 < sc.P && sc.bundle_start.size() % 4 != 0) {  // idle bundles up to the next stream's first one (never executed)
                sc.bundle_start.push_back((uint32_t)sc.order.size());
                sc.bundle_coop.push_back(0);
                sc.bundle_flags.push_back(0);
            }
        }
    }
    const uint32_t NB = (uint32_t)sc.bundle_start.size();
    sc.bundle_start.push_back((uint32_t)sc.order.size());
    if ((uint64_t)NB * G * 16ull > 0xffffffffull) {  // the record stream is addressed through one 32-bit buffer window
        err = "graph too large: " + std::to_string(NB) + " bundles of " + std::to_string(G) + " records exceed the 4 GiB record window";
        return false;
    }
    return true;
}

// ---- operand routing -------------------------------------------------------------------------------
// RING: produced at most RING_BUNDLES bundles ago (any node slot) -> read from the wave's result ring in LDS.
// MEM : everything else (older values, constants, every third operand) -> its slot in the tile, staged into LDS
//       OPND_AHEAD bundles ahead.  The staging load of bundle b is issued while bundle b - OPND_AHEAD runs, i.e.
//       before that bundle stores: a MEM operand must be at least OPND_AHEAD + 1 bundles old, which the ring
//       depth guarantees.  A value that is neither a witness element nor read through MEM is never given a
//       slot (its store goes to the tile's trash slot).
static_assert(RING_BUNDLES >= OPND_AHEAD, "values younger than the staging distance must come from the ring");
enum { SRC_MEM = 0, SRC_RING = 1 };
static uint32_t route(const Graph& g, const Schedule& sc, uint32_t producer, uint32_t consumer, int q) {
    if ((q >= 2 && g.nodes[consumer].kind != N_FUSED && g.nodes[consumer].kind != N_SCAN) || g.nodes[producer].kind == N_CONST) return SRC_MEM;  // (TernCond reads its third operand in place)
    if (sc.stream_of[producer] != sc.stream_of[consumer]) return SRC_MEM;  // (another wave's ring)
    const uint32_t d = sc.use_bundle_of[consumer] - sc.bundle_of[producer];
    return (d >= 1 && d <= RING_BUNDLES) ? SRC_RING : SRC_MEM;
}
// the collect half of a division served by the divider wave: no operands
static bool is_collect(const Graph& g, uint32_t divider, uint32_t entry) { return divider && !(entry & REQ_FLAG) && class_of(g.nodes[entry]) == C_DIV; }

struct Routing {
    std::vector<uint32_t> pos_in_bundle;  // record position of every scheduled node
    std::vector<uint32_t> last_mem_use;   // last bundle that reads the value from memory
    std::vector<uint8_t> needs_slot;      // 1: read through memory, 2: pinned (a witness element, or read by another stream)
};

static Routing route_operands(const Graph& g, const Schedule& sc, uint32_t divider) {
    const size_t N = g.nodes.size();
    const uint32_t NB = (uint32_t)sc.bundle_start.size() - 1;
    Routing rt;
    rt.pos_in_bundle.assign(N, 0);
    for (uint32_t b = 0; b < NB; ++b)
        for (uint32_t k = sc.bundle_start[b]; k < sc.bundle_start[b + 1]; ++k) rt.pos_in_bundle[sc.order[k] & ~REQ_FLAG] = sc.order_pos[k];
    rt.last_mem_use.assign(N, 0);
    rt.needs_slot.assign(N, 0);
    for (uint32_t w : g.witness_signals)
        if (g.nodes[w].kind != N_CONST) rt.needs_slot[w] = 2;  // pinned
    for (uint32_t e : sc.order) {
        if (is_collect(g, divider, e)) continue;
        const uint32_t i = e & ~REQ_FLAG;
        const Node& n = g.nodes[i];
        // Neg is encoded as 0 - a: its operand travels in the b position
        const uint32_t ops[3] = {n.a, n.b, n.c};
        for (int q = 0; q < arity_of(n); ++q) {
            const uint32_t o = ops[q];
            if (n.kind == N_SCAN && q == 1 && g.nodes[o].kind != N_CONST && sc.stream_of[o] == sc.stream_of[i] && sc.bundle_of[o] == sc.use_bundle_of[i]) continue;  // (the accumulator arrives inside the bundle)
            if (g.nodes[o].kind == N_CONST || route(g, sc, o, i, q) != SRC_MEM) continue;
            if (!rt.needs_slot[o]) rt.needs_slot[o] = 1;
            if (sc.stream_of[o] != sc.stream_of[i]) rt.needs_slot[o] = 2;  // read by another stream: the slot is never reused
            rt.last_mem_use[o] = std::max(rt.last_mem_use[o], sc.use_bundle_of[i]);
        }
    }
    return rt;
}

// (A DIV step names its constant 2^k only through the side table scan_imm -- the Mul node that read it is gone --, and the general path
// multiplies with that constant's Montgomery form: whatever passes run between the rewrite and here must have kept and renumbered it.)
static bool check_scan_div_bases(const Graph& g, const NodeForms& f, std::string& err) {
    const size_t N = g.nodes.size();
    for (size_t i = 0; i < N; ++i)
        if (g.nodes[i].kind == N_SCAN && (g.nodes[i].op & SCAN_OP_DIV)) {
            const uint32_t c = i < f.scan_imm.size() ? f.scan_imm[i] : 0xffffffffu;
            bool pow2 = c < N && g.nodes[c].kind == N_CONST;
            if (pow2) {
                const Fr& v = g.const_values[g.nodes[c].a];
                int bits = 0;
                for (int w = 0; w < 8; ++w) bits += __builtin_popcount(v.v[w]);
                pow2 = bits == 1;
            }
            if (!pow2) {
                err = "internal error: a division step's base is not a constant power of two";
                return false;
            }
        }
    return true;
}

static uint32_t sub_of(uint8_t op) {
    switch (op) {
        case OP_ADD: return SUB_ADD;   case OP_SUB: return SUB_SUB;   case OP_MUL: return SUB_MULT;
        case OP_EQ: return SUB_EQ;     case OP_NEQ: return SUB_NEQ;   case OP_LAND: return SUB_LAND; case OP_LOR: return SUB_LOR;
        case OP_LT: return SUB_LT;     case OP_GT: return SUB_GT;     case OP_LEQ: return SUB_LEQ;   case OP_GEQ: return SUB_GEQ;
        case OP_SHL: return SUB_SHL;   case OP_SHR: return SUB_SHR;   case OP_BOR: return SUB_BOR;   case OP_BAND: return SUB_BAND;
        case OP_BXOR: return SUB_BXOR; case OP_IDIV: return SUB_IDIV; case OP_MOD: return SUB_MOD;
        case OP_BITX: return SUB_BITX;
        default: return 0;  // Div: the class says it all
    }
}

// ---- slot allocation (LIFO free list: a just-freed slot is still hot in cache) + encoding ----
// Slot numbering inside a tile: constants first (index = constant index), then value slots, then the trash slot.
struct Encoder {
    const Graph& g; const NodeForms& f; const Schedule& sc; const Routing& rt; ConstTable& ct; Program& out;
    const uint32_t T, G, divider, NC;
    const size_t n_in_buf;
    const uint64_t slot_bytes;
    const bool witness_slots, nowhere;
    const uint32_t zero_off;
    uint32_t cref_row = 0;  // one row of G words per C_INPUT / C_TERN bundle, in bundle order (the interpreter counts rows)
    uint32_t n_slots = 0;
    std::vector<uint32_t> free_slots;
    std::vector<uint32_t> witness_rank;
    std::vector<uint8_t> ctrl_of;  // record -> ctrl, kept aside until the destinations are known
    std::vector<uint32_t> dying;   // nodes whose slot is released after the current bundle
    uint64_t stream_class_bundles[MAX_STREAMS][C_COUNT] = {};
    uint64_t stream_bitx[MAX_STREAMS] = {0, 0, 0, 0}, stream_riders[MAX_STREAMS] = {0, 0, 0, 0};
    double stream_form_saved[MAX_STREAMS] = {0, 0, 0, 0};
    uint32_t s_cref[MAX_STREAMS] = {0, 0, 0, 0};  // rows of the third-operand / input-index table in front of each stream
    uint32_t scan_run = 0, scan_longest = 0, scan_bits = 0;  // scan bundles: the current / the longest chain segment, kind and shift

    uint64_t mem_off(uint32_t producer) const {
        if (g.nodes[producer].kind == N_CONST) return (uint64_t)(ct.ref[producer] & ~REF_CONST) * slot_bytes;
        return ((uint64_t)NC + ct.ref[producer]) * slot_bytes;
    }
    bool encode_node(uint32_t b, uint32_t k, bool request, bool collect, bool fusedb, uint32_t rep, uint32_t stage, std::string& err);
    void header_bits(uint32_t b, int cl, uint32_t rep, uint32_t form_bits, uint32_t stream, uint32_t& lin_bits, double& form_saved);
    bool encode_bundles(std::string& err);
    void finish();
};

// the records of the node at order[k] in bundle b (position order_pos[k])
bool Encoder::encode_node(uint32_t b, uint32_t k, bool request, bool collect, bool fusedb, uint32_t rep, uint32_t stage, std::string& err) {
    const uint32_t k0 = sc.bundle_start[b];
    const uint32_t i = sc.order[k] & ~REQ_FLAG;
    const Node& n = g.nodes[i];
    const uint32_t js = sc.order_pos[k];  // node slot (record position)
    uint32_t slot = 0xffffffffu;
    if (rt.needs_slot[i] && !request) {
        if (witness_slots && witness_rank[i] != 0xffffffffu) {
            slot = witness_rank[i];
        } else if (!free_slots.empty()) {
            slot = free_slots.back();
            free_slots.pop_back();
        } else {
            slot = n_slots++;
        }
    }
    if (!request) ct.ref[i] = slot;  // 0xffffffff: no slot (every use comes from the ring)
    uint32_t r[4] = {0, 0, slot, 0};
    // default: both operands unused -> staging loads of the zero constant, LDS reads of the own stage cells
    uint32_t off[2] = {zero_off, zero_off};
    uint32_t lds[2] = {stage + js * rep * T * 16u, stage + 2u * LDS_HALF_BYTES + js * rep * T * 16u};  // (C_MULQ: value t + T * js is loaded by lane 4 * T * js + t)
    // operand `producer` (operand number q of the node): its ring cell, or its slot for the staging load into the own stage cell
    auto enc_to = [&](uint32_t producer, int q, uint32_t& off_out, uint32_t& lds_out) {
        if (route(g, sc, producer, i, q) == SRC_RING) {
            lds_out = LDS_RING_OFF + (sc.bundle_of[producer] % RING_BUNDLES) * RING_SLOT_BYTES + rt.pos_in_bundle[producer] * T * 16u;
        } else {
            const uint64_t o = g.nodes[producer].kind == N_CONST && reads_canonical_constants(g, f, i, q) ? (uint64_t)ct.canon_const[producer] * slot_bytes : mem_off(producer);
            off_out = (uint32_t)o;
        }
    };
    auto enc_operand = [&](uint32_t producer, int q) { enc_to(producer, q, off[q], lds[q]); };
    uint32_t ctrl = CTRL_ACTIVE;
    if (fusedb) {
        // main record (positions 4j, 4j+2): the product's factors, destination, op2; extra record (4j+1, 4j+3): the
        // operands of the second and third stage, op3.  A plain multiplication rides with op2 = op3 = none.
        const bool is_f = n.kind == N_FUSED, sq = is_f && fused_sq(n.op);
        const uint32_t op2 = is_f ? fused_op2(n.op) : FOP_NONE, op3 = is_f ? fused_op3(n.op) : FOP_NONE;
        const uint32_t px = js * rep + 1u;  // the extra record's position: its own stage cells
        uint32_t xoff[2] = {zero_off, zero_off};
        uint32_t xlds[2] = {stage + px * T * 16u, stage + 2u * LDS_HALF_BYTES + px * T * 16u};
        enc_to(n.a, 0, off[0], lds[0]);
        if (sq) {
            enc_to(n.a, 0, off[1], lds[1]);
            if (op2) enc_to(n.b, 1, xoff[0], xlds[0]);
            if (op3) enc_to(n.c, 2, xoff[1], xlds[1]);
        } else {
            enc_to(n.b, 1, off[1], lds[1]);
            if (op2) enc_to(n.c, 2, xoff[0], xlds[0]);
        }
        const uint32_t rm[4] = {off[0], off[1], slot, lds[0] | (lds[1] << 16)};
        const uint32_t rx[4] = {xoff[0], xoff[1], 0xffffffffu, xlds[0] | (xlds[1] << 16)};
        for (uint32_t x = 0; x < rep; ++x) {
            memcpy(&out.recs[((size_t)b * G + js * rep + x) * 4], (x & 1u) ? rx : rm, sizeof rm);
            ctrl_of[(size_t)b * G + js * rep + x] = (uint8_t)(CTRL_ACTIVE | ((x & 1u) ? op3 : op2));
        }
        const uint32_t fops[3] = {n.a, n.b, n.c};
        for (int q = 0; q < arity_of(n); ++q)
            if (rt.needs_slot[fops[q]] == 1 && rt.last_mem_use[fops[q]] == b) dying.push_back(fops[q]);
        return true;
    }
    if (!collect)
    switch (n.kind) {
        case N_INPUT:
            if (n.a >= n_in_buf) {
                err = "Input index out of range";
                return false;
            }
            out.crefs[(size_t)cref_row * G + js] = n.a;  // input index
            break;
        case N_UNO:  // Neg(a) = 0 - a  (graph.rs:188-194: 0 -> 0, else r - a); a travels in the b position
            ctrl |= SUB_SUB;
            enc_operand(n.a, 1);
            break;
        case N_DUO:
            ctrl |= sub_of(n.op);
            enc_operand(n.a, 0);
            if (n.op == OP_BITX) {  // the shift amount travels in the b_lds field, no second operand is read
                lds[1] = g.const_values[g.nodes[n.b].a].v[0] * 16u;
                break;
            }
            enc_operand(n.b, 1);
            break;
        case N_SCAN: {
            // position 2p: the step's OUT record {x, accumulator at a chain's head}; 2p + 1: its ACC record {divisor, 2^k in Montgomery form} (DIV)
            const bool is_acc = (n.op & SCAN_OP_ACC) != 0, is_div = (n.op & SCAN_OP_DIV) != 0;
            if ((js & 1u) != (is_acc ? 1u : 0u)) {
                err = "internal error: scan records out of place";
                return false;
            }
            const uint32_t pair = js / 2;
            const bool is_sel = scan_is_sel(n.op);
            const bool start = pair == 0 || is_sel || (n.op & SCAN_OP_NOACC) || (sc.order[k0 + 2 * pair - 1] & ~REQ_FLAG) != n.b;
            ctrl |= (is_acc ? SCAN_ROLE_ACC : 0u) | (start ? SCAN_START : 0u);
            if (!is_acc) {
                if (!(n.op & SCAN_OP_NOX)) enc_operand(n.a, 0);  // (a chain end without this operand reads 0: the record's default)
                if (start && !(n.op & SCAN_OP_NOACC)) enc_operand(n.b, 1);
                scan_run = start ? 1u : scan_run + 1u;
                scan_longest = std::max(scan_longest, scan_run);
                scan_bits = (is_div ? HDR_SCAN_DIV : 0u) | ((n.op & SCAN_OP_BORROW) ? HDR_SCAN_BORROW : 0u) | ((n.op & SCAN_OP_LEX) ? HDR_SCAN_LEX : 0u) |
                            ((n.op & SCAN_OP_KG) ? HDR_SCAN_KG : 0u) | ((n.op & SCAN_OP_KL) ? HDR_SCAN_KL : 0u) | (scan_shift_of(g, f, i) << HDR_SCAN_SHIFT_SHIFT);
            } else if (is_sel) {  // the ACC record: the selection's arms p, q
                enc_operand(n.a, 0);
                enc_operand(n.b, 1);
            } else if (is_div) {
                enc_to(n.c, 2, off[0], lds[0]);
                off[1] = (uint32_t)mem_off(f.scan_imm[i]);
            } else if (scan_has_third(n.op)) {  // BORROW / LEX: y
                enc_to(n.c, 2, off[0], lds[0]);
            }
            break;
        }
        case N_CONV:
            if (js != (f.scan_imm[i] & 0xffu)) {
                err = "internal error: convolution columns out of place";
                return false;
            }
            enc_operand(n.a, 0);
            enc_operand(n.b, 1);
            scan_bits = HDR_SCAN_CONV;
            scan_longest = f.scan_imm[i] >> 8;  // (k rounds)
            break;
        case N_TRES:
            enc_operand(n.a, 0);
            enc_operand(n.b, 1);
            out.crefs[(size_t)cref_row * G + js] = g.nodes[n.c].kind == N_CONST && reads_canonical_constants(g, f, i, 2) ? (uint32_t)((uint64_t)ct.canon_const[n.c] * slot_bytes)
                                                                                                                     : (uint32_t)mem_off(n.c);  // third operand always through memory
            break;
    }
    r[0] = off[0];
    r[1] = off[1];
    r[3] = lds[0] | (lds[1] << 16);
    for (uint32_t x = 0; x < rep; ++x) {
        memcpy(&out.recs[((size_t)b * G + js * rep + x) * 4], r, sizeof r);
        ctrl_of[(size_t)b * G + js * rep + x] = (uint8_t)ctrl;
    }
    const uint32_t ops[3] = {n.a, n.b, n.c};
    for (int q = 0; q < (collect ? 0 : arity_of(n)); ++q) {
        uint32_t o = ops[q];
        if (rt.needs_slot[o] == 1 && rt.last_mem_use[o] == b) dying.push_back(o);
    }
    return true;
}

// the header bits of bundle b that depend on all of its nodes, and the cycles its form saves against the class's price
void Encoder::header_bits(uint32_t b, int cl, uint32_t rep, uint32_t form_bits, uint32_t stream, uint32_t& lin_bits, double& form_saved) {
    const uint32_t k0 = sc.bundle_start[b], k1 = sc.bundle_start[b + 1];
    ProgramStats& st = out.stats;
    if (cl == C_MULF) {  // which stages any node of the bundle has (the kernel runs those for every group)
        for (uint32_t k = k0; k < k1; ++k) {
            const uint32_t op2 = ctrl_of[(size_t)b * G + (k - k0) * rep] & CTRL_SUB_MASK, op3 = ctrl_of[(size_t)b * G + (k - k0) * rep + 1] & CTRL_SUB_MASK;
            lin_bits |= (op2 == FOP_MUL ? HDR_F_S2MUL : op2 ? HDR_F_S2LIN : 0u) | (op3 ? HDR_F_S3LIN : 0u);
        }
        form_saved = (lin_bits & HDR_F_S2MUL ? 0.0 : kCyclesFusedStageMul) + ((lin_bits & (HDR_F_S2LIN | HDR_F_S3LIN)) ? 0.0 : kCyclesFusedStageLin);
    }
    if (cl == C_SCAN) {
        lin_bits = scan_bits | ((scan_longest - 1u) << HDR_SCAN_ITER_SHIFT);
        const bool limbs64 = ((scan_bits >> HDR_SCAN_SHIFT_SHIFT) & 0xffu) == 64u && scan_longest > 2;  // (priced as the parallel forms: what limb-sized operands take)
        uint32_t log_rounds = 0;
        while ((1u << log_rounds) < scan_longest) ++log_rounds;
        const double scan_cycles = (scan_bits & HDR_SCAN_CONV) ? kCyclesConvFront + (double)scan_longest * kCyclesConvStep
                                   : (scan_bits & (HDR_SCAN_BORROW | HDR_SCAN_LEX)) ? kCyclesScanFront + kCyclesScanBits
                                   : (scan_bits & HDR_SCAN_DIV) ? kCyclesScanFrontDiv + (limbs64 ? kCyclesScanParDivFlat + log_rounds * kCyclesScanParDivRound : (double)scan_longest * kCyclesScanStepDiv)
                                                                : kCyclesScanFront + (limbs64 ? kCyclesScanParCarry : (double)scan_longest * kCyclesScanStepCarry);
        form_saved = kCycles[C_SCAN] - scan_cycles;
    }
    if (cl == C_LIN || cl == C_MUL || cl == C_MULQ)
        for (uint32_t k = k0; k < k1; ++k) {
            const uint32_t sub = ctrl_of[(size_t)b * G + (k - k0) * rep] & CTRL_SUB_MASK;
            lin_bits |= sub == SUB_SUB ? HDR_LIN_SUB : sub == SUB_ADD ? HDR_LIN_ADD : 0u;
        }
    if (cl == C_MUL && k1 > k0 && (f.vflags[sc.order[k0] & ~REQ_FLAG] & VF_MUL_CC)) {  // canonical products (a heap of their own: all or none)
        lin_bits |= HDR_MUL_CC;
        form_saved = kCycles[C_MUL] - kCyclesMulCC;
    }
    if (cl == C_BIT) {
        bool all = true;
        for (uint32_t k = k0; k < k1; ++k) all = all && (ctrl_of[(size_t)b * G + (k - k0)] & CTRL_SUB_MASK) == SUB_BITX;
        bool limb_ops = true, any_shr = false;  // Shr and Band nodes only: the straight path
        for (uint32_t k = k0; k < k1; ++k) {
            const uint32_t sub = ctrl_of[(size_t)b * G + (k - k0)] & CTRL_SUB_MASK;
            limb_ops = limb_ops && (sub == SUB_SHR || sub == SUB_BAND);
            any_shr = any_shr || sub == SUB_SHR;
        }
        lin_bits |= !limb_ops ? 0u : any_shr ? HDR_BIT_ALL_SHR : HDR_BIT_ALL_BAND;
        if (all) {
            lin_bits |= HDR_BITX_ALL;
            st.n_bitx_bundles++;
            stream_bitx[stream]++;
            form_saved = form_bits & HDR_A_CANON ? kCyclesBitxOperandForm : 0.0;
        }
    }
    if (cl == C_BIT && (lin_bits & (HDR_BIT_ALL_SHR | HDR_BIT_ALL_BAND)) && !(lin_bits & HDR_BITX_ALL))  // (straight path: measured with every form canonical)
        form_saved = (form_bits & HDR_A_CANON ? kCyclesOperandForm : 0.0) + (form_bits & HDR_B_CANON ? kCyclesOperandForm : 0.0) +
                     (form_bits & HDR_OUT_CANON ? kCyclesResultForm : 0.0) + kCyclesBitStraight;
    else if (is_integer_class(cl) && !(lin_bits & HDR_BITX_ALL))
        form_saved = (form_bits & HDR_A_CANON ? kCyclesOperandForm : 0.0) + (form_bits & HDR_B_CANON ? kCyclesOperandForm : 0.0) +
                     ((form_bits & HDR_OUT_CANON) && cl != C_CMPS ? kCyclesResultForm : 0.0);
}

// first pass: slots bundle by bundle; r = {a_off, b_off, slot id (patched by finish), a_lds | b_lds << 16}, ctrl kept aside
bool Encoder::encode_bundles(std::string& err) {
    const uint32_t NB = (uint32_t)sc.bundle_start.size() - 1;
    ProgramStats& st = out.stats;
    ctrl_of.assign((size_t)NB * G, 0);
    for (uint32_t b = 0; b < NB; ++b) {
        const uint32_t k0 = sc.bundle_start[b], k1 = sc.bundle_start[b + 1], cnt = k1 - k0;
        const bool idle = cnt == 0;  // (programs of several streams: padding around the posts and waits; an Add of zeros into the trash slot)
        const bool request = !idle && (sc.order[k0] & REQ_FLAG) != 0, collect = !idle && is_collect(g, divider, sc.order[k0]);
        const bool coop = sc.bundle_coop[b] == 1 || sc.bundle_coop[b] == 2, fusedb = sc.bundle_coop[b] == 2;
        const uint32_t rep = coop ? COOP_LANES : 1u;  // a C_MULQ / C_MULF node's records take COOP_LANES positions (4j .. 4j+3)
        const int cl = idle ? (sc.bundle_flags[b] ? (int)C_SYNC : (int)C_LIN) : request ? (int)C_DIVREQ : collect ? (int)C_DIVGET : fusedb ? (int)C_MULF : coop ? (int)C_MULQ : class_of(g.nodes[sc.order[k0]]);
        uint32_t stream = 0;
        while (stream + 1 < sc.P && b >= sc.s_first[stream + 1]) ++stream;
        if (b == sc.s_first[stream]) free_slots.clear();  // a slot is reused inside the stream that freed it only (the others run at their own pace)
        const bool executed = b < sc.s_first[stream] + sc.s_count[stream];  // (not the never-executed padding in front of the next stream)
        if (executed) {
            st.class_bundles[cl]++;
            st.class_nodes[cl] += cnt;
            stream_class_bundles[stream][cl]++;
        }
        dying.clear();
        const uint32_t stage = LDS_STAGE_OFF + (b % OPND_AHEAD) * STAGE_BYTES;
        if (b == sc.s_first[stream]) s_cref[stream] = cref_row;
        const bool has_crefs = cl == C_INPUT || cl == C_TERN;
        if (has_crefs) out.crefs.resize((size_t)(cref_row + 1) * G, 0);
        // integer-class bundles: which operands arrive as canonical integers, and whether the result stays one
        uint32_t form_bits = 0;
        if (!idle && cl == C_INPUT && (f.vflags[sc.order[k0] & ~REQ_FLAG] & VF_OUT_CANON)) form_bits |= HDR_OUT_CANON;  // (bit graphs: every Input node)
        if (!idle && (is_integer_class(cl) || cl == C_CMPZ)) {
            const uint8_t f0 = f.vflags[sc.order[k0] & ~REQ_FLAG];
            for (uint32_t k = k0; k < k1; ++k) {
                const uint8_t fk = f.vflags[sc.order[k] & ~REQ_FLAG];
                if ((cl == C_CMPZ ? (fk ^ f0) & VF_OUT_CANON : (fk ^ f0)) != 0) {
                    err = "internal error: operand forms differ inside a bundle";
                    return false;
                }
            }
            if (cl != C_CMPZ) form_bits |= (f0 & VF_A_CANON ? HDR_A_CANON : 0u) | (f0 & VF_B_CANON ? HDR_B_CANON : 0u);
            form_bits |= f0 & VF_OUT_CANON ? HDR_OUT_CANON : 0u;
        }
        scan_run = scan_longest = scan_bits = 0;
        for (uint32_t k = k0; k < k1; ++k)
            if (!encode_node(b, k, request, collect, fusedb, rep, stage, err)) return false;
        if (cl == C_MUL && !idle && (f.vflags[sc.order[k0] & ~REQ_FLAG] & VF_MUL_CC))
            for (uint32_t k = k0; k < k1; ++k)
                if (!(f.vflags[sc.order[k] & ~REQ_FLAG] & VF_MUL_CC) || class_of(g.nodes[sc.order[k] & ~REQ_FLAG]) != C_MUL) {
                    err = "internal error: canonical and Montgomery products in one bundle";
                    return false;
                }
        uint32_t lin_bits = 0;
        double form_saved = 0;
        header_bits(b, cl, rep, form_bits, stream, lin_bits, form_saved);
        if (executed) {
            st.form_cycles_saved += (uint64_t)form_saved;
            stream_form_saved[stream] += form_saved;
        }
        if (cl == C_MULQ && lin_bits) {
            st.n_coop_rider_bundles++;
            stream_riders[stream]++;
        }
        out.hdr[b] = (uint32_t)cl | (cnt << HDR_COUNT_SHIFT) | lin_bits | form_bits | sc.bundle_flags[b];
        if (has_crefs) {  // (inactive node slots repeat the first word: a valid input index / slot offset)
            for (uint32_t q = cnt; q < G; ++q) out.crefs[(size_t)cref_row * G + q] = out.crefs[(size_t)cref_row * G];
            ++cref_row;
        }
        std::sort(dying.begin(), dying.end());
        dying.erase(std::unique(dying.begin(), dying.end()), dying.end());
        for (uint32_t o : dying) free_slots.push_back(ct.ref[o]);
    }
    n_slots = std::max(n_slots, 1u);
    if (ws_tile_bytes(NC, n_slots, T) >= (uint64_t)OFF_NOWHERE) {
        err = "graph too large: one tile of the value workspace exceeds the 4 GiB buffer range";
        return false;
    }
    return true;
}

// second pass: destination byte offsets (trash slot = n_slots) + ctrl, and inactive padding records; then the streams' prices
void Encoder::finish() {
    const uint32_t NB = (uint32_t)sc.bundle_start.size() - 1;
    const uint32_t trash_off = nowhere ? OFF_NOWHERE : (uint32_t)(((uint64_t)NC + n_slots) * slot_bytes);
    out.trash_off = trash_off;
    for (uint32_t b = 0; b < NB; ++b) {
        const uint32_t rep = sc.bundle_coop[b] == 1 || sc.bundle_coop[b] == 2 ? COOP_LANES : 1u;
        const uint32_t cnt = (sc.bundle_start[b + 1] - sc.bundle_start[b]) * rep;  // record positions in use
        const uint32_t stage = LDS_STAGE_OFF + (b % OPND_AHEAD) * STAGE_BYTES;
        for (uint32_t q = 0; q < cnt; ++q) {
            uint32_t* r = &out.recs[((size_t)b * G + q) * 4];
            const uint32_t d = r[2] == 0xffffffffu ? trash_off : (uint32_t)(((uint64_t)NC + r[2]) * slot_bytes);
            r[2] = d | ctrl_of[(size_t)b * G + q];
        }
        for (uint32_t q = cnt; q < G; ++q) {  // inactive node slots: harmless operands, store -> trash, not ACTIVE
            uint32_t* r = &out.recs[((size_t)b * G + q) * 4];
            r[0] = r[1] = zero_off;
            r[2] = trash_off | (sc.bundle_coop[b] == 2 ? 0u : ctrl_of[(size_t)b * G] & CTRL_SUB_MASK);  // (fused bundles: idle groups have no second / third stage)
            const uint32_t cell = (q / rep) * rep * T * 16u;  // (C_MULQ: the four positions of an idle group read one zero cell)
            r[3] = (stage + cell) | ((stage + 2u * LDS_HALF_BYTES + cell) << 16);
        }
    }
    out.n_slots = n_slots;
    out.n_streams = sc.P;
    out.n_cref_rows = cref_row;
    for (uint32_t s = 0; s < MAX_STREAMS; ++s) {
        out.stream_first[s] = sc.s_first[s];
        out.stream_count[s] = sc.s_count[s];
        out.stream_div_requests[s] = sc.s_div[s];
        out.stream_cref_first[s] = s < sc.P && sc.s_count[s] ? s_cref[s] : cref_row;
        double c = 0, heavy = 0;
        for (int k = 0; k < (int)C_COUNT; ++k) c += kCycles[k] * (double)stream_class_bundles[s][k];
        c += kCyclesCoopRiders * (double)stream_riders[s] - (kCycles[C_BIT] - kCyclesBitx) * (double)stream_bitx[s] - stream_form_saved[s];
        for (int k : {(int)C_MUL, (int)C_MULQ, (int)C_MULF, (int)C_DIV}) heavy += kCycles[k] * (double)stream_class_bundles[s][k];
        out.stream_cycles[s] = c;
        out.stream_chain_cycles[s] = sc.s_chain[s];
        out.stream_cycles_mul_div[s] = heavy;
    }
}

static bool allocate_and_encode(const Graph& g, const NodeForms& f, const Schedule& sc, const Routing& rt, ConstTable& ct, const uint32_t* class_cost, const Knobs& k,
                                uint32_t divider, size_t n_in_buf, Program& out, std::string& err) {
    const uint32_t T = out.T, G = out.G, NB = (uint32_t)sc.bundle_start.size() - 1;
    out.hdr.resize(NB);
    out.recs.assign((size_t)NB * G * 4, 0);
    out.crefs.clear();
    // Witness-ordered slots: the pinned slot of a witness element is its rank among the witness
    // list's distinct nodes, so the output gather (pack kernel) reads consecutive memory and every 128-byte line it
    // fetches is used whole (tiles of one or two sets have 32- / 64-byte slots: with slots in schedule order the two
    // halves of a line are fetched at different times, 1.56 x the algorithmic read volume measured in round 2).  The
    // interpreter's stores / staging loads of such values then scatter: fine where it is bound by instruction issue,
    // 15 % slower on the wide, memory-heavier sha256 graph (round 1) -- hence a policy.
    // Default (round 4): on for tiles of one or two sets of graphs that are not linear-heavy -- measured neutral for the
    // authV2-class interpreter (12.54 ms either way at 1024 sets, profiles/r03_pack_ab.txt) while the pack kernel's reads drop
    // from 1.43 x to 1.0 x the algorithmic volume; CWC_WITNESS_SLOTS=0 / 1 forces either way.
    const bool witness_slots = k.witness_slots.value_or(T <= 2 && class_cost != kClassCostLinHeavy);
    const uint64_t slot_bytes = 32ull * T;
    Encoder enc{g, f, sc, rt, ct, out, T, G, divider, out.n_const, n_in_buf, slot_bytes, witness_slots, k.nowhere,
                k.nowhere ? OFF_NOWHERE : (uint32_t)((uint64_t)ct.zero_const * slot_bytes)};
    if (witness_slots) {
        enc.witness_rank.assign(g.nodes.size(), 0xffffffffu);
        for (uint32_t w : g.witness_signals)
            if (g.nodes[w].kind != N_CONST && enc.witness_rank[w] == 0xffffffffu) enc.witness_rank[w] = enc.n_slots++;
    }
    if (!check_scan_div_bases(g, f, err) || !enc.encode_bundles(err)) return false;
    enc.finish();
    out.n_inputs = (uint32_t)n_in_buf;
    out.n_witness = (uint32_t)g.witness_signals.size();
    out.witness_refs.resize(out.n_witness);
    for (size_t i = 0; i < g.witness_signals.size(); ++i) {
        const uint32_t w = g.witness_signals[i];
        out.witness_refs[i] = ct.ref[w] | (g.nodes[w].kind != N_CONST && f.rep[w] == REP_C ? REF_CANON : 0u);
    }
    return true;
}

static bool compile_variant(const Graph& g_in, uint32_t T, uint32_t divider, bool bit_fusion, const VariantOptions& opt, const Knobs& k, Program& out,
                            std::string& err, RewriteCache* cache, bool probe_only, uint32_t streams) {
    if (streams != 1 && streams != 2 && streams != 4) {
        err = "a tile is evaluated by 1, 2 or 4 streams";
        return false;
    }
    if (T == 0 || T > 64 || (T & (T - 1))) {
        err = "tile width must be a power of two in 1..64";
        return false;
    }
    PhaseTimer phase{k.debug_compile_times, T};
    PreparedGraph pg;
    if (!prepare_graph(g_in, T, divider, bit_fusion, opt, k, cache, probe_only, phase, out, pg, err)) return false;
    Graph& g = pg.g;
    ProgramStats& st = out.stats;
    if (probe_only) {
        for (const Node& n : g.nodes)  // (nodes per class of the graph as loaded: the runtime asks whether there are divisions)
            if (n.kind != N_CONST && class_of(n) >= 0) st.class_nodes[class_of(n)]++;
        out.n_inputs = (uint32_t)pg.n_in_buf;
        out.n_witness = (uint32_t)g.witness_signals.size();
        return true;
    }
    phase("rewrites");
    const NodeForms forms = choose_forms(g, T, divider, opt, k, pg.class_cost, phase, st);
    st.chain_floor_cycles = chain_floor(g);
    ConstTable ct = build_constant_table(g, forms, out);
    phase("constants");
    Schedule sc;
    if (!schedule_program(g, forms, st, pg.class_cost, opt, k, T, divider, streams, cache && cache->lock, sc, err)) return false;
    out.n_bundles = (uint32_t)sc.bundle_start.size() - 1;
    out.div_lanes = std::move(sc.div_lanes);
    out.n_div_requests = sc.n_div_requests;
    phase("schedule");
    if (k.debug_node_mix) dump_node_mix(g, T);
    const Routing rt = route_operands(g, sc, divider);
    phase("routing");
    if (!allocate_and_encode(g, forms, sc, rt, ct, pg.class_cost, k, divider, pg.n_in_buf, out, err)) return false;
    phase("slots + encoding");
    return true;
}

}  // namespace cwc
