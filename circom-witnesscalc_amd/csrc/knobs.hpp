// Every environment variable libcircom_witnesscalc_amd.so reads, as one snapshot.  An extern "C" entry point calls
// read_knobs() on its caller's thread before any work and hands the snapshot down as `const Knobs&`; whatever runs on
// another thread (candidate compiles, the background refinement, parse / write / copy workers) holds a copy made on the
// caller's thread.  knobs.cc is the only file that reads the environment.  (One exception: the cost model's global cycle table is
// built from a snapshot taken when the library is loaded -- costmodel.cc.)
// An unset optional: the variable is not set.  "set": the variable exists, whatever its value.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <optional>
#include <string>

namespace cwc {

struct Knobs {
    // ---- graph compiler: schedule variants (compile.cc compile_program) ----
    std::optional<uint32_t> coop_fill;   // CWC_COOP_FILL, unset: force the narrow-bundle policy's fill
    std::optional<uint32_t> coop_slack;  // CWC_COOP_SLACK, unset: force the narrow-bundle policy's slack
    bool no_coop_mul;                    // CWC_NO_COOP_MUL, off: no narrow multiplication bundles
    bool no_schedule_variants;           // CWC_NO_SCHEDULE_VARIANTS, off: one schedule, no search
    bool no_bit_fusion;                  // CWC_NO_BIT_FUSION, off: no bit-extract fusion
    bool no_rep_inference;               // CWC_NO_REP_INFERENCE, off: every value in Montgomery form
    bool conv_always;                    // CWC_CONV_ALWAYS, off: the program without convolution bundles does not compete
    bool no_fuse;                        // CWC_NO_FUSE, off: no fused narrow chains
    std::optional<uint32_t> fuse;        // CWC_FUSE, unset: the one fused-chain policy tried, whatever it costs
    // ---- graph compiler: one variant (compile.cc) ----
    std::optional<bool> witness_slots;   // CWC_WITNESS_SLOTS, unset: force witness-ordered slots on (non-zero) / off (0)
    bool debug_compile_times;            // CWC_DEBUG_COMPILE_TIMES, off: seconds per phase on stderr
    bool no_load_optimize;               // CWC_NO_LOAD_OPTIMIZE, off: skip the load-time optimiser
    bool random_eval;                    // CWC_RANDOM_EVAL, 0: random-evaluation passes in front of the load-time optimiser
    bool no_lin_heavy_weights;           // CWC_NO_LIN_HEAVY_WEIGHTS, off: linear-heavy graphs keep the plain weight table
    std::optional<uint32_t> sched_lin_cost;  // CWC_SCHED_LIN_COST, unset: the scheduler's weight of a linear bundle
    std::optional<uint32_t> sched_mul_cost;  // CWC_SCHED_MUL_COST, unset: the scheduler's weight of a multiplication bundle
    bool no_tree_reduction;              // CWC_NO_TREE_REDUCTION, off: no tree-height reduction
    std::optional<size_t> tree_leaves;   // CWC_TREE_LEAVES, unset (8, or 64 at T = 1): leaves per rebalanced tree, at least 2
    bool no_scan;                        // CWC_NO_SCAN, off: no scan bundles (also: the program-size bound counts plain depth)
    bool no_bit_graph;                   // CWC_NO_BIT_GRAPH, off: bit graphs are not given canonical inputs and products
    bool no_mul_cc;                      // CWC_NO_MUL_CC, off: no canonical limb products
    bool no_conv;                        // CWC_NO_CONV, off: no convolution bundles
    uint32_t sched_div_wait = 3;         // CWC_SCHED_DIV_WAIT, 3: (measured 3 against 6 and 10: +1.4 % at 1024 sets and +2.6 % at 2048 with divider waves, +1.4 % at 8192 and 16384 sets with inline inversions)
    bool sched_tie_reverse;              // CWC_SCHED_TIE_REVERSE, off: ties among ready nodes against file order
    bool no_ride_along;                  // CWC_NO_RIDE_ALONG, off: no linear riders in multiplication bundles
    bool scan_eager;                     // CWC_SCAN_EAGER, off: scan bundles are emitted as soon as a step is ready
    double stream_prologue = 30000;      // CWC_STREAM_PROLOGUE, 30000: (cycles of dependent operations from the inputs that still count as prologue)
    bool debug_critical_path;            // CWC_DEBUG_CRITICAL_PATH, off: class composition of the critical path on stderr
    bool debug_streams;                  // CWC_DEBUG_STREAMS, off: the streams' parts and cycles on stderr
    bool debug_node_mix;                 // CWC_DEBUG_NODE_MIX, off: what the scheduled graph is made of on stderr
    uint32_t debug_sched = 0;            // CWC_DEBUG_SCHED, 0: the first n bundles, node by node, on stderr
    bool nowhere = true;                 // CWC_NOWHERE, 1: (0: the zero constant's slot and the trash slot as before round 4, for A/B runs)
    // ---- graph compiler: the exact rewrites (rewrite.cc) ----
    std::optional<bool> tree_inner_skip;  // CWC_TREE_INNER_SKIP, unset (graphs beyond 16 M nodes): skip inner chain nodes in the tree-height reduction
    bool debug_scan;                     // CWC_DEBUG_SCAN, off: what the scan detection found on stderr
    bool no_scan_ends;                   // CWC_NO_SCAN_ENDS, off: chain ends and carry-chain tails stay outside the scan bundles
    bool no_bit_scans;                   // CWC_NO_BIT_SCANS, off: no borrow / comparison / selection scans
    bool sel_always;                     // CWC_SEL_ALWAYS, 0: selection scans also in graphs without borrow / comparison steps
    bool no_sel_cmp;                     // CWC_NO_SEL_CMP, off: selections do not take their ordered comparison along
    bool no_sel_nez;                     // CWC_NO_SEL_NEZ, off: other TernCond nodes stay in the TernCond class
    bool no_sel_scans;                   // CWC_NO_SEL_SCANS, off: no selection scans
    bool conv_any_width;                 // CWC_CONV_ANY_WIDTH, off: convolution bundles for factors of any width (tests)
    bool debug_conv;                     // CWC_DEBUG_CONV, off: what the convolution detection found on stderr
    bool conv_skip_dependency_check;     // CWC_CONV_SKIP_DEPENDENCY_CHECK, off: (tests of compile_program's fallback)
    // ---- program choice (pipeline.cc) ----
    std::optional<uint32_t> tile_width;  // CWC_TILE_WIDTH, unset: the program key of every batch (width, + 256 for the divider wave)
    size_t target_waves = 2048;          // CWC_TARGET_WAVES, 2048: the static rule widens tiles beyond this many waves
    size_t divider_tiles = 1024;         // CWC_DIVIDER_TILES, 1024: divider waves up to this many tiles
    double program_mb = 960.0;           // CWC_PROGRAM_MB, 960: the tile width is raised until the program stream fits
    bool static_tile_rule;               // CWC_STATIC_TILE_RULE, off: the static rule's key, no cost model
    bool no_quick_first_call;            // CWC_NO_QUICK_FIRST_CALL, off: small batches wait for the full choice too
    bool no_group_divider;               // CWC_NO_GROUP_DIVIDER, off: no candidates with one divider per three / four waves
    bool no_streams;                     // CWC_NO_STREAMS, off: no candidates with several streams
    bool debug_cost;                     // CWC_DEBUG_COST, off: the cost model's price of every candidate on stderr
    std::optional<double> pack_pass_cycles;  // CWC_PACK_PASS_CYCLES, unset (2300): cycles of a pack pass in the pack schedule's replay, at least 1
    // ---- launches (pipeline.cc) ----
    bool force_mode3;                    // CWC_FORCE_MODE3, off: (layout experiments: any limb program in the MODE 3 instances)
    std::optional<int> stream_tiles_per_workgroup;  // CWC_STREAM_TILES_PER_WORKGROUP, unset (2 beyond 256 tiles): tiles of a two-stream divider program per workgroup
    std::optional<int> waves_per_workgroup;         // CWC_WAVES_PER_WORKGROUP, unset (by tile count): 1 or 4 interpreter waves per workgroup
    double workspace_gb = 8.0;           // CWC_WORKSPACE_GB, 8: bytes of one value workspace chunk
    long streams = 0;                    // CWC_STREAMS, 0 (all that fit): cap on the workspace chunks of one launch
    std::optional<int> inline_pack;      // CWC_INLINE_PACK, unset (1): rows the divider waves pack: 0 none, 1 the schedule's prefix, 2 all that are ever ready
    std::optional<uint32_t> inline_pack_rows;  // CWC_INLINE_PACK_ROWS, unset: (measurements: a cap on the divider waves' share)
    bool pack_v1;                        // CWC_PACK_V1, off: the first pack kernel at every tile width
    int pack = 3;                        // CWC_PACK, 3: (2: one thread per slot, the round-2 shape, for A/B)
    // ---- host threads and transfers (pipeline.cc, capi_batch.cc) ----
    unsigned parse_threads;              // CWC_PARSE_THREADS, every core: threads that parse input sets
    unsigned write_threads;              // CWC_WRITE_THREADS, up to 16: threads that write .wtns files
    unsigned copy_threads;               // CWC_COPY_THREADS, up to 16: threads that move witness rows out of the staging buffers
    size_t copy_slice_mb = 32;           // CWC_COPY_SLICE_MB, 32: slice of the host-rows witness copy (1..1024)
    size_t e2e_subbatch = 1024;          // CWC_E2E_SUBBATCH, 1024: input sets per sub-batch of the streaming entry point
    size_t e2e_slice_mb = 96;            // CWC_E2E_SLICE_MB, 96: slice of the streaming entry point's witness copy (1..1024)
    // ---- the single-shot entry point (capi_single.cc) ----
    std::string cache_dir;               // CWC_PROGRAM_CACHE, else $XDG_CACHE_HOME or $HOME/.cache, /circom-witnesscalc-amd: the program cache's directory; "", 0, off or no home: empty, no cache
    bool no_warm_thread;                 // CWC_NO_WARM_THREAD, off: the device is not brought up on a thread of its own
    bool debug_single;                   // CWC_DEBUG_SINGLE, off: where a call's time goes on stderr
    bool debug_cache;                    // CWC_DEBUG_CACHE, off: program cache hits and writes on stderr
    bool quirks;                         // GW_REFERENCE_QUIRKS, off (unset, empty or 0): the reference's prints and its status quirk (lib.rs:106-108)
    // ---- the cost model's cycle table (costmodel.cc; read when the library is loaded) ----
    std::optional<std::string> model_cycles;       // CWC_MODEL_CYCLES, unset: "class:cycles,..." over the built-in table
    std::optional<std::string> model_cycles_file;  // CWC_MODEL_CYCLES_FILE, unset (model_cycles.txt in cache_dir): the calibration file
};
Knobs read_knobs();

}  // namespace cwc
