// read_knobs(): the one reader of the process environment (knobs.hpp).
#include "knobs.hpp"

#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <thread>

namespace cwc {

Knobs read_knobs() {
    auto on = [](const char* name) { return getenv(name) != nullptr; };
    auto u32 = [](const char* name) -> std::optional<uint32_t> {
        if (const char* e = getenv(name)) return (uint32_t)atol(e);
        return std::nullopt;
    };
    // a thread count: the variable when it is positive, else every core up to `cap` (0: no cap)
    const long cores = (long)std::thread::hardware_concurrency();
    auto threads = [cores](const char* name, long cap) {
        long v = 0;
        if (const char* e = getenv(name)) v = atol(e);
        if (v <= 0) v = cap && cores > cap ? cap : cores;
        return v < 1 ? 1u : (unsigned)v;
    };
    // megabytes of a copy slice: the variable when it lies in 1..1024
    auto slice_mb = [](const char* name, size_t dflt) {
        if (const char* e = getenv(name)) {
            const long v = atol(e);
            if (v >= 1 && v <= 1024) return (size_t)v;
        }
        return dflt;
    };
    Knobs k = {};
    k.coop_fill = u32("CWC_COOP_FILL"), k.coop_slack = u32("CWC_COOP_SLACK"), k.no_coop_mul = on("CWC_NO_COOP_MUL");
    k.no_schedule_variants = on("CWC_NO_SCHEDULE_VARIANTS"), k.no_bit_fusion = on("CWC_NO_BIT_FUSION"), k.no_rep_inference = on("CWC_NO_REP_INFERENCE");
    k.conv_always = on("CWC_CONV_ALWAYS"), k.no_fuse = on("CWC_NO_FUSE");
    if (const char* e = getenv("CWC_FUSE")) k.fuse = (uint32_t)atoi(e);
    if (const char* e = getenv("CWC_WITNESS_SLOTS")) k.witness_slots = atoi(e) != 0;
    k.debug_compile_times = on("CWC_DEBUG_COMPILE_TIMES"), k.no_load_optimize = on("CWC_NO_LOAD_OPTIMIZE");
    if (const char* e = getenv("CWC_RANDOM_EVAL")) k.random_eval = atoi(e) != 0;
    k.no_lin_heavy_weights = on("CWC_NO_LIN_HEAVY_WEIGHTS");
    if (const char* e = getenv("CWC_SCHED_LIN_COST")) k.sched_lin_cost = (uint32_t)atoi(e);
    if (const char* e = getenv("CWC_SCHED_MUL_COST")) k.sched_mul_cost = (uint32_t)atoi(e);
    k.no_tree_reduction = on("CWC_NO_TREE_REDUCTION");
    if (const char* e = getenv("CWC_TREE_LEAVES")) k.tree_leaves = (size_t)std::max(2, atoi(e));
    k.no_scan = on("CWC_NO_SCAN"), k.no_bit_graph = on("CWC_NO_BIT_GRAPH"), k.no_mul_cc = on("CWC_NO_MUL_CC"), k.no_conv = on("CWC_NO_CONV");
    if (const char* e = getenv("CWC_SCHED_DIV_WAIT")) k.sched_div_wait = (uint32_t)atoi(e);
    k.sched_tie_reverse = on("CWC_SCHED_TIE_REVERSE"), k.no_ride_along = on("CWC_NO_RIDE_ALONG"), k.scan_eager = on("CWC_SCAN_EAGER");
    if (const char* e = getenv("CWC_STREAM_PROLOGUE")) k.stream_prologue = atof(e);
    k.debug_critical_path = on("CWC_DEBUG_CRITICAL_PATH"), k.debug_streams = on("CWC_DEBUG_STREAMS"), k.debug_node_mix = on("CWC_DEBUG_NODE_MIX");
    if (const char* e = getenv("CWC_DEBUG_SCHED")) k.debug_sched = (uint32_t)atoi(e);
    if (const char* e = getenv("CWC_NOWHERE")) k.nowhere = atoi(e) != 0;

    if (const char* e = getenv("CWC_TREE_INNER_SKIP")) k.tree_inner_skip = atoi(e) != 0;
    k.debug_scan = on("CWC_DEBUG_SCAN"), k.no_scan_ends = on("CWC_NO_SCAN_ENDS"), k.no_bit_scans = on("CWC_NO_BIT_SCANS");
    if (const char* e = getenv("CWC_SEL_ALWAYS")) k.sel_always = atoi(e) != 0;
    k.no_sel_cmp = on("CWC_NO_SEL_CMP"), k.no_sel_nez = on("CWC_NO_SEL_NEZ"), k.no_sel_scans = on("CWC_NO_SEL_SCANS");
    k.conv_any_width = on("CWC_CONV_ANY_WIDTH"), k.debug_conv = on("CWC_DEBUG_CONV"), k.conv_skip_dependency_check = on("CWC_CONV_SKIP_DEPENDENCY_CHECK");

    if (const char* e = getenv("CWC_TILE_WIDTH")) k.tile_width = (uint32_t)atoi(e);
    if (const char* e = getenv("CWC_TARGET_WAVES")) {
        const long v = atol(e);
        if (v > 0) k.target_waves = (size_t)v;
    }
    if (const char* e = getenv("CWC_DIVIDER_TILES")) k.divider_tiles = (size_t)atol(e);
    if (const char* e = getenv("CWC_PROGRAM_MB")) k.program_mb = atof(e);
    k.static_tile_rule = on("CWC_STATIC_TILE_RULE"), k.no_quick_first_call = on("CWC_NO_QUICK_FIRST_CALL");
    k.no_group_divider = on("CWC_NO_GROUP_DIVIDER"), k.no_streams = on("CWC_NO_STREAMS"), k.debug_cost = on("CWC_DEBUG_COST");
    if (const char* e = getenv("CWC_PACK_PASS_CYCLES")) k.pack_pass_cycles = std::max(1.0, atof(e));

    k.force_mode3 = on("CWC_FORCE_MODE3");
    if (const char* e = getenv("CWC_STREAM_TILES_PER_WORKGROUP")) k.stream_tiles_per_workgroup = atoi(e);
    if (const char* e = getenv("CWC_WAVES_PER_WORKGROUP")) k.waves_per_workgroup = atoi(e);
    if (const char* e = getenv("CWC_WORKSPACE_GB")) k.workspace_gb = atof(e);
    if (const char* e = getenv("CWC_STREAMS")) k.streams = atol(e);
    if (const char* e = getenv("CWC_INLINE_PACK")) k.inline_pack = atoi(e);
    if (const char* e = getenv("CWC_INLINE_PACK_ROWS")) k.inline_pack_rows = (uint32_t)atol(e);
    k.pack_v1 = on("CWC_PACK_V1");
    if (const char* e = getenv("CWC_PACK")) k.pack = atoi(e);

    k.parse_threads = threads("CWC_PARSE_THREADS", 0);  // (round 2 capped this at 16 threads: 27 k sets/s on a 256-core host)
    k.write_threads = threads("CWC_WRITE_THREADS", 16);  // (more writers fight the copy engine for host memory bandwidth: 64 -> 9.4 k, 32 -> 13.9 k, 16 -> 15.5 k witnesses/s, r03_e2e_ab.txt)
    k.copy_threads = threads("CWC_COPY_THREADS", 16);
    k.copy_slice_mb = slice_mb("CWC_COPY_SLICE_MB", 32), k.e2e_slice_mb = slice_mb("CWC_E2E_SLICE_MB", 96);
    if (const char* e = getenv("CWC_E2E_SUBBATCH")) {
        const long v = atol(e);
        if (v >= 1) k.e2e_subbatch = (size_t)v;
    }

    // the program cache's directory: CWC_PROGRAM_CACHE=<dir> names it, CWC_PROGRAM_CACHE= / 0 / off turns the cache off;
    // default $XDG_CACHE_HOME or ~/.cache, /circom-witnesscalc-amd
    if (const char* e = getenv("CWC_PROGRAM_CACHE")) {
        if (*e && strcmp(e, "0") && strcmp(e, "off")) k.cache_dir = e;
    } else {
        const char *x = getenv("XDG_CACHE_HOME"), *home = getenv("HOME");
        if (x && *x) k.cache_dir = std::string(x) + "/circom-witnesscalc-amd";
        else if (home && *home) k.cache_dir = std::string(home) + "/.cache/circom-witnesscalc-amd";
    }
    k.no_warm_thread = on("CWC_NO_WARM_THREAD"), k.debug_single = on("CWC_DEBUG_SINGLE"), k.debug_cache = on("CWC_DEBUG_CACHE");
    if (const char* e = getenv("GW_REFERENCE_QUIRKS")) k.quirks = *e && strcmp(e, "0") != 0;

    if (const char* e = getenv("CWC_MODEL_CYCLES")) k.model_cycles = e;
    if (const char* e = getenv("CWC_MODEL_CYCLES_FILE")) k.model_cycles_file = e;
    return k;
}

}  // namespace cwc
