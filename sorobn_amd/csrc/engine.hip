// mibn engine: C-ABI (include/mibn.h) over the planner and the gfx950 kernels.
// No CPU fallback: every query entry point needs a live HIP device.
#include <hip/hip_runtime.h>
#include <dlfcn.h>
#include <rccl/rccl.h>  // types and prototypes only: librccl.so is dlopen'ed by mibn_comm_init, never linked

#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <memory>
#include <mutex>
#include <numeric>
#include <string>
#include <thread>
#include <utility>
#include <vector>

#include "../../include/mibn.h"
#include "device_mem.h"
#include "gibbs_kernel.hip.h"
#include "bp_kernel.hip.h"
#include "sample_kernel.hip.h"
#include "count_kernel.hip.h"
#include "count_weighted_kernel.hip.h"
#include "score_kernel.hip.h"
#include "citest_kernel.hip.h"
#include "dag_kernel.hip.h"
#include "dag_post_kernel.hip.h"
#include "planner.h"
#include "plan_policy.h"
#include "tiny_kernel.hip.h"
#include "sweep_kernel.hip.h"
#include "ve_kernel.hip.h"
#include "draw_kernel.hip.h"
#include "elim_kernel.hip.h"
#include "expect_kernel.hip.h"
#include "likelihood_kernel.hip.h"
#include "wave_plan_kernel.hip.h"

using namespace mibn;

namespace {
double now_ms() {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}
}  // namespace

// ---------------------------------------------------------------------------------------------- device order search
// The elimination-order search of the planner (order_search.h - the same code the host runs) as a kernel: one request
// per lane, the search state in a global buffer.  Pure bit-set / integer work, independent per request and latency-bound:
// it occupies a few hundred wave slots for a few milliseconds beside the level kernels and takes ~40 % of the planning
// time off the host cores (option "gpu_search").
struct OrderArgs {
    OrderNet net;
    const int64_t *q_off, *e_off;
    const int32_t *q_vars, *e_vars;
    int64_t B;
    uint32_t flags;
    uint8_t *orders;       // [B][128]
    int32_t *order_len;    // [B]
    OrderScratch *scratch; // [B]
    uint32_t *zero;        // a counter the launch resets (emit_kernel's item cursor: no memset on the planning stream), or null
    const int32_t *perm;   // [B] or null: lane position -> request of the slice (requests of similar size share a wave: plan_on_device_launch)
    int32_t lanes;         // requests per wave (the other lanes of the 64 leave at once: the lanes of a wave run different requests -
                           // every data-dependent branch diverges - so a wave's time grows with the lanes in use; fewer lanes in more
                           // waves finish sooner, as long as the chip has SIMDs to spare: option plan_lanes)
};

// (Workgroups of up to 16 waves - no cooperation between them, only placement: the waves of a workgroup share a CU, so the 512
// waves of a chunk take 32 CUs whole instead of one workgroup's worth of registers on every CU - beside the level and sweep
// kernels, whose workgroups fill a CU's register file exactly, that is an eighth of the chip instead of a third to a half.)
#ifndef MIBN_ORDER_WAVES_PER_EU
#define MIBN_ORDER_WAVES_PER_EU 4  // build-time experiment hooks: the register budget of the planner's kernels (waves per SIMD)
#endif
#ifndef MIBN_EMIT_WAVES_PER_EU
#define MIBN_EMIT_WAVES_PER_EU 4
#endif
#ifndef MIBN_PLAN_WG
#define MIBN_PLAN_WG 1024  // largest workgroup of the planner's kernels (option plan_waves x 64 must not exceed it)
#endif
__global__ __launch_bounds__(MIBN_PLAN_WG, MIBN_ORDER_WAVES_PER_EU) void order_kernel(const OrderArgs A) {
    if (A.zero && blockIdx.x == 0 && threadIdx.x == 0) *A.zero = 0;
    const int lane = (int)(threadIdx.x & 63), wave = (int)(threadIdx.x >> 6), waves = (int)(blockDim.x >> 6);
    if (lane >= A.lanes) return;
    const int64_t pos = ((int64_t)blockIdx.x * waves + wave) * A.lanes + lane;
    if (pos >= A.B) return;
    const int64_t b = A.perm ? A.perm[pos] : pos;
    OrderScratch &S = A.scratch[pos];
    const int64_t q0 = A.q_off[b], e0 = A.e_off[b];
    order_search(A.net, S, (int)(A.q_off[b + 1] - q0), A.q_vars + q0, (int)(A.e_off[b + 1] - e0), A.e_vars + e0,
                 (A.flags & MIBN_Q_NOPRUNE) != 0);
    uint8_t *out = A.orders + b * 128;
    for (int i = 0; i < S.n_best; ++i) out[i] = S.best[i];
    A.order_len[b] = S.n_best;
}

// Device program emission (emit_core.h: the code the host's planning workers run): one request per lane turns its elimination
// order (order_kernel's output, never copied to the host) into its step program, written straight into the request's slot
// of the chunk's device program buffer, and cuts it into work items.  The host only lays out the schedule of the chunk
// (build_schedule, from the work items): a rank needs no planning threads.
struct EmitArgs {
    EmitNet net;
    const int64_t *q_off, *e_off, *out_off;  // [B + 1]; out_off relative to the chunk's first request
    const int32_t *q_vars, *e_vars, *e_codes;
    const char *skip;                        // [B] evidence outside the domain: zero steps
    const uint8_t *orders;                   // [B][128]
    const int32_t *order_len;                // [B]
    int64_t B;
    uint32_t flags;
    uint32_t *prog;                          // [B][prog_stride]
    uint32_t prog_stride;
    EmitMeta *meta;                          // [B]
    Tag *tags;                               // [tag_cap]: the work items of all requests, a request's contiguous
    uint32_t *tag_cursor;
    uint32_t tag_cap;
    char *scratch;                           // [B][scratch_stride] planning state (EmitScratch)
    size_t scratch_stride;
    const int32_t *perm;                     // [B] or null (see OrderArgs)
    int32_t lanes;                           // requests per wave (see OrderArgs)
};

#if defined(MIBN_EMIT_PROF)
__device__ unsigned long long g_emit_prof[12];  // 100 MHz ticks per phase, summed over the lanes (see MIBN_TICK in emit_core.h)
#endif

__global__ __launch_bounds__(MIBN_PLAN_WG, MIBN_EMIT_WAVES_PER_EU) void emit_kernel(const EmitArgs A) {
    const int lane = (int)(threadIdx.x & 63), wave = (int)(threadIdx.x >> 6), waves = (int)(blockDim.x >> 6);
    if (lane >= A.lanes) return;
    const int64_t pos = ((int64_t)blockIdx.x * waves + wave) * A.lanes + lane;
    if (pos >= A.B) return;
    const int64_t b = A.perm ? A.perm[pos] : pos;
    EmitMeta m;
    m.words = 1; m.n_tags = 0; m.tag_first = 0; m.err = 0; m.prog_first = 0; m.pad_ = 0;
    m.alg_bytes = m.alg_flops = m.n_steps = m.max_step_cells = 0;
    m.arena_cells = 0;
    uint32_t *slot = A.prog + (size_t)b * A.prog_stride;
    if (A.skip[b]) { slot[0] = 0; A.meta[b] = m; return; }
#if defined(MIBN_EMIT_PROF)
    EmitProf prof_;
    for (int k = 0; k < 12; ++k) prof_.a[k] = 0;
#if defined(__HIP_DEVICE_COMPILE__)
    prof_.t = __builtin_amdgcn_s_memrealtime();
#endif
#endif
    EmitScratch S;
    emit_scratch_carve(S, A.scratch + (size_t)pos * A.scratch_stride, A.net.n_vars);
    const int64_t q0 = A.q_off[b], e0 = A.e_off[b];
    const int nq = (int)(A.q_off[b + 1] - q0), ne = (int)(A.e_off[b + 1] - e0);
    int err = emit_begin(A.net, S, nq, A.q_vars + q0, ne, A.e_vars + e0, A.e_codes + e0, (A.flags & MIBN_Q_NOPRUNE) != 0);
    EmitBuf buf;
    buf.data = slot;
    buf.cap = A.prog_stride;
    EmitStats st;
    MIBN_TICK(0)  // relevant set, evidence-sliced CPTs
    if (!err) err = emit_run(A.net, S, buf, st, nullptr, nq, A.q_vars + q0, A.out_off[b], A.orders + b * 128, (int)A.order_len[b] MIBN_PROF_PASS);
    if (!err) {
        const uint32_t nt = tag_program(A.net, slot, [](const Tag &) {});
        const uint32_t first = atomicAdd(A.tag_cursor, nt);
        if (first + nt <= A.tag_cap) {
            uint32_t k = first;
            tag_program(A.net, slot, [&](const Tag &t) { A.tags[k++] = t; });
            m.n_tags = nt;
            m.tag_first = first;
        } else {
            err = kEmitErrWords;
        }
    }
    MIBN_TICK(10)  // work items
#if defined(MIBN_EMIT_PROF)
    for (int k = 0; k < 12; ++k) atomicAdd(&g_emit_prof[k], prof_.a[k]);
#endif
    m.err = err;
    m.words = (uint32_t)buf.size;
    m.alg_bytes = st.alg_bytes; m.alg_flops = st.alg_flops; m.n_steps = st.n_steps; m.max_step_cells = st.max_step_cells;
    m.arena_cells = st.arena_cells;
    A.meta[b] = m;
}

// Chunk sets (pinned program buffers, device copies, schedule, launch events): with n sets in use the host plans chunk
// k + n - 1 at the earliest when chunk k has completed.  Two by default.  With two sets and a call of three chunks the
// second chunk of a call can only be planned once the previous call has finished - the GPU runs the short first chunk and
// then idles 5-12 ms (the "[mibn gap]" lines of option trace); a third set (option chunk_sets=3) closes those gaps but
// proved erratic end to end (planning wall time doubles, runs between 155 k and 204 k queries/s against a steady
// 194-204 k with two: profiles/r02_q_chunk_sets.log), so it stays an experiment.
constexpr int kChunkSets = 4;
// Streams of a wave's level launches (LevelStreams; the column `stream` of kLevelKernels): the lane's own and its three aux streams.
constexpr int kLevelStreams = 4;
// statistics slots: the classes of work (split_kinds: 0 .. kNumKernels - 1, kernel_name), then the kernels of mibn_query_batch as
// launched, the two of mibn_mpe_batch, the one of mibn_expect_batch, the two phases of mibn_score_families and the two of
// mibn_posterior_sample_batch, the two of mibn_map_batch and - no kernels: what ve_map_kernel's launches held - its tiled sum and max
// steps, and the reduction of mibn_ci_tests (ci_lane_kernel, ci_wave_kernel and ci_finish_kernel together), and the two kernels of a call with likelihood
// findings: the seeds of a planned wave, the tiny kernel's twin, the one kernel of mibn_bp_batch, the one of mibn_bp_mpe_batch and the two of mibn_bp_evidence_batch,
// the weighted counting, the two phases of mibn_best_dag and the four of mibn_arc_posteriors.  Order and names are what mibn_last_kernel_stats reports: a new slot goes to the end of both lists.
enum StatSlot : int {
    kStatLevel = kNumKernels, kStatTiny, kStatSweepDma, kStatPlanner, kStatLevelGroup, kStatSegment, kStatMfma, kStatMax, kStatTraceback,
    kStatExpect, kStatCount, kStatScore, kStatSum, kStatDraw, kStatMap, kStatMapTraceback, kStatMapSumTiles, kStatMapMaxTiles, kStatCiTest, kStatSeed, kStatTinyLh, kStatBp, kStatBpMax, kStatBpEvidence, kStatBpAccumulate, kStatCountW, kStatDagSubset, kStatDagSink,
    kStatDagPostSubset, kStatDagPostLevel, kStatDagPostSuperset, kStatDagPostArc, kStatSlots
};
constexpr const char *kStatSlotNames[kStatSlots - kNumKernels] = {
    "ve_level_kernel", "tiny_kernel", "ve_sweep_dma_kernel", "order_kernel+emit_kernel",
    "level:ve_level_kernel||ve_mfma_kernel||ve_sweep_dma_kernel||ve_segment_kernel", "ve_segment_kernel", "ve_mfma_kernel", "ve_max_kernel",
    "mpe_traceback_kernel", "expect_kernel", "count_kernel", "score_kernel", "ve_sum_kernel", "posterior_draw_kernel",
    "ve_map_kernel", "map_traceback_kernel", "ve_map_kernel:sum tiles", "ve_map_kernel:max tiles", "citest_kernel", "likelihood_seed_kernel", "tiny_lh_kernel", "bp_kernel", "bp_max_kernel", "bp_evidence_kernel", "bp_accumulate_kernel", "count_weighted_kernel", "dag_subset_kernel", "dag_sink_kernel",
    "dag_post_subset_kernel", "dag_post_level_kernel", "dag_post_superset_kernel", "dag_post_arc_kernel"};
// mibn_score_families: cells of the device buffer its count tables are written to (8 bytes each, 32 MiB).  A sweep of hill climbing over
// 100 four-state columns with up to three parents - 10 000 families of at most 256 cells, 2.6 M cells at worst - fits one sub-batch, so
// the usual call is one counting and one scoring launch; zeroing the buffer takes microseconds at HBM rate, and it stays negligible
// beside the 288 GB of the device.  A single larger table (up to 2^28 cells) gets a sub-batch - and a buffer - of its own.
constexpr int64_t kScoreCellBudget = int64_t(1) << 22;

// Likelihood findings of a batch (mibn_set_likelihoods): the caller's CSR block, copied.
struct Findings {
    int64_t B = 0;
    std::vector<int64_t> l_off, v_off;  // l_off[B + 1] over l_vars; v_off[n + 1] over values
    std::vector<int32_t> l_vars;
    std::vector<double> values;
    bool any() const { return !l_vars.empty(); }
};
// The seeds of one chunk of such a call (likelihood_kernel.hip.h): the records of its requests - none for a request no program runs
// for - and where each request's begin, host and device.  One per chunk set and one for run_elim: live until the chunk's last wave ran.
struct ChunkSeeds {
    std::vector<SeedRec> recs;
    std::vector<uint32_t> first;  // [n + 1]: the records of request r of the chunk are recs[first[r] .. first[r + 1])
    DevBuf<SeedRec> d_recs;
    DevBuf<double> d_values;
    PinnedBuf stage[2];
};

struct mibn_ctx {
    Network net;
    bool has_net = false;
    bool planner_only = false;
    int device = -1;
    int n_cu = 0;
    // (members are destroyed in reverse order: the streams come first here, so every buffer and event below is freed before them)
    Stream stream;       // kernels, gibbs, result download
    Stream copy_stream;  // program / schedule uploads: overlap the previous chunk's kernels
    Stream stream2;      // lane 1 (lane 0 = stream)
    Stream aux[2][kLevelStreams - 1];  // option overlap, per lane: the sweep kernel's, the segment kernel's and the MFMA kernel's launches
    Stream search_stream;  // the device planner's (plan_stream)
    DevBuf<double> d_pool;
    // Lanes: consecutive chunks of a call alternate between two streams with an arena each and run CONCURRENTLY - requests are
    // independent, and the launch boundaries of one chunk's levels (the only synchronisation of the level-synchronous schedule)
    // then overlap with the other chunk's launches instead of leaving the tail of every launch to half-empty CUs.
    DevBuf<char> d_arena[2];      // private arenas of the requests of the wave in flight, per lane (sized in bytes: grow_arena)
    double *arena(int lane) const { return reinterpret_cast<double *>(d_arena[lane].get()); }
    DevBuf<double> d_results[2];  // dense posteriors of the call in flight (two calls may overlap)
    struct Pending {                            // an asynchronous call whose results have not been collected yet
        bool active = false;
        double *out = nullptr;
        size_t cells = 0;
        Event done;
    } pend[2];
    int next_slot = 0;
    // chunk pipeline: workers plan the next chunks into pinned buffers while the GPU runs chunk i
    std::unique_ptr<ThreadPool> pool;
    struct Set {
        PinnedBuf stage[4];         // prog_off, arena_off, items, wg_item
        std::vector<ProgBuf> bufs;  // pinned host program buffers, one per worker
        std::vector<ProgBuf> xbufs; // ... and the ones the host re-plans single requests of a device-planned chunk into (beyond a device limit)
        BatchPlan xplan;
        DevBuf<uint32_t> d_prog;
        DevBuf<uint64_t> d_prog_off, d_arena_off;
        DevBuf<uint32_t> d_wg_item;
        DevBuf<Item> d_items;
        Event uploaded;                      // the copy stream has delivered this set's programs and schedule
        std::vector<Event> ev;               // launch boundaries of the waves in flight
        struct Timed {  // kid >= 0: one launch, booked to that statistics slot, between the events e[0]; kWave: the wall time of a wave
                        // (kernel_ms), e[0] too; kLevelGroup: the launches of one level on the streams of option overlap, as ONE concurrent
                        // launch group - e[s] brackets the launch on stream s (kNone: the level has none there); its duration is the span
                        // from the earliest start to the latest end
            enum Kind : int { kWave = -1, kLevelGroup = -2 };
            static constexpr size_t kNone = ~size_t(0);
            int kid; size_t e[kLevelStreams][2]; double bytes, items; uint64_t call;
            Timed(int kid_, size_t e0, size_t e1, double bytes_, double items_, uint64_t call_) : kid(kid_), bytes(bytes_), items(items_), call(call_) {
                for (auto &p : e) p[0] = p[1] = kNone;
                e[0][0] = e0; e[0][1] = e1;
            }
        };
        std::vector<Timed> timed;
        size_t ev_used = 0;
        bool busy = false;
        int gap_from = -1;  // trace: index (in mibn_ctx::gap_ev) of the event that closed the previous wave
        BatchPlan plan;
        Schedule sched;
        std::vector<LaunchGroup> groups;  // the launches of `sched`
        ChunkSeeds seeds;                 // a call with likelihood findings
        ~Set() {  // (ProgBuf is planner.h's, shared with the host tools: its backing is freed here)
            for (auto *v : {&bufs, &xbufs})
                for (ProgBuf &b : *v) {
                    if (b.grow) (void)PinnedBuf::adopt(b.data).release();  // (pinned_grow's)
                    b.release();
                }
        }
    } set[kChunkSets];
    PinnedBuf res_stage[2];  // pinned landing buffers of asynchronous calls
    // small-network specialisation (tiny_kernel.hip.h): one lane per request, no planning
    bool tiny_ok = false;
    int tiny = 1;              // option: 1 = use it where the network is eligible, 0 = always plan step programs
    int tiny_zero_copy = 1;    // option: calls of at most kTinyZeroCopyRequests requests read / write pinned host memory directly (run_tiny)
    DevBuf<int32_t> d_tiny_meta;
    int32_t tiny_meta_words = 0;
    DevBuf<char> d_tiny_req;  // request arrays of the call in flight
    PinnedBuf tiny_stage;
    PlanPolicy pol;                  // the adaptive planning policy and the share rule of the device planner (plan_policy.h)
    int second_on_device = 0;        // option: 1 = device-planned calls emit the runner-up too (tests: the wave planner's second emission)
    double retired_requests = 0;     // requests whose kernel time has been booked (the unit of kernel_ms in the policy's windows)
    // device order search (order_kernel)
    int plan_lanes = 0;              // requests per wave of order_kernel / emit_kernel (1..64); 0 = by the rank's planning threads: plan_lanes_now()
    int plan_waves = 16;             // waves per workgroup of the two (1..16): see order_kernel
    int plan_sort = 0;               // experiment (off): the requests of a slice dealt to the lanes by descending relevant-set size - 1: consecutive
                                     // ranks share a wave; 2: round-robin over the workgroups (every CU the same mix, homogeneous waves); 3: round-
                                     // robin over the waves (every wave the same sum).  Measured at 24 lanes per wave, two planning threads
                                     // (profiles/r05_h/i/j_*.log): 250 k queries/s unsorted, 231 k (1), 231 k (2), 249 k (3) - homogeneous waves
                                     // are the slow ones: the lanes of a wave diverge almost completely, a wave's time is the SUM of its lanes',
                                     // and the stream's own order already mixes the sizes; balancing the sums exactly (3) shortens the
                                     // planner's kernels by 2 % and moves nothing.  32 lanes, four threads: 259 / 265 / 265 / 258 k.
    int gpu_search = 0;              // option: 1 = search elimination orders on the device (networks of <= 128 variables)
    DevBuf<char> d_order_net;        // the OrderNet arrays
    OrderNet order_net_dev;          // pointers into d_order_net
    bool order_net_ok = false;
    DevBuf<uint8_t> d_orders;
    DevBuf<int32_t> d_order_len;
    DevBuf<OrderScratch> d_order_scratch;
    PinnedBuf search_in, search_out;  // pinned: request arrays in, orders + lengths out
    double search_ms = 0;            // host wall time spent waiting for the device search (last call)
    // device program emission (emit_kernel)
    int gpu_emit = 0;                // option: 1 = the device plans whole chunks (order search + emission), 2 = the same, checked
                                     // word for word against the host's planner (tests)
    DevBuf<char> d_emit_net;         // the EmitNet arrays
    EmitNet emit_net_dev;            // pointers into d_emit_net
    bool emit_net_ok = false;
    DevBuf<char> d_emit_scratch;     // planning state, one slice per lane
    DevBuf<uint32_t> d_emit_cursor;
    DevBuf<uint32_t> d_plan_perm;     // the order in which wave_plan_kernel's waves draw the requests of a chunk (plan_sort_kernel: the long ones first)
    int wave_sort = 1;                // option: 0 = by index
    PinnedBuf emit_in, emit_out;     // pinned, read / written by the kernels themselves: request arrays in, per-request results and work items out
    Event emit_ev[2];                // around the planner's kernels
    BatchPlan emit_dev, emit_host;   // the two parts of a chunk before they are joined
    uint32_t emit_words = 6144;      // words of a request's program slot (doubles after a chunk that did not fit)
    int64_t emit_single = 0;         // requests of device-planned chunks the host planned because they exceeded a device limit
    // wave-cooperative device planner (wave_plan_kernel)
    int wave_plan = 1;               // option: 1 = chunks the device plans go through wave_plan_kernel where the network is covered (wave_plan.h)
    int plan_priority = 2;           // option: the device planner's stream priority (2 highest - the default since round 4 -, 1 normal, 0 lowest); before the first device-planned chunk
    int wave_wgs = 0;                // option: workgroups of a wave_plan_kernel launch (0: one per four requests - the whole chip at once)
    std::unique_ptr<WNet> wnet_host;  // the packed network + options as uploaded last
    DevBuf<WNet> d_wnet;
    bool wnet_ok = false;
    double emit_ms = 0;              // host wall time spent waiting for the device planner (last call)
    uint64_t emit_chunks = 0, emit_fallbacks = 0;
    Event gap_ev[4];          // trace: ends of the last waves (GPU idle time between waves)
    uint64_t n_waves = 0;
    int n_sets = 2;           // chunk sets in use (option "chunk_sets": 2..4; two per lane: one on the GPU, one being planned)
    int set_cursor = 0;    // the chunk set the next chunk plans into: alternates across calls, so that a call of one chunk
                           // plans into the idle set while the previous call's kernels still run from the other one
    uint64_t call_id = 0;  // kernel time retired later is booked to the call that launched it
    // RCCL (multi-GPU gather / reduce), loaded on demand
    struct Comm {
        Stream stream;  // collectives run on their own stream: the gather of batch s must not queue behind the
                        // kernels of batch s + 1, which the two-deep pipeline has already submitted
        void *dl = nullptr;
        ncclComm_t comm = nullptr;
        int rank = 0, world = 1;
        decltype(&ncclGetUniqueId) GetUniqueId = nullptr;
        decltype(&ncclCommInitRank) CommInitRank = nullptr;
        decltype(&ncclCommDestroy) CommDestroy = nullptr;
        decltype(&ncclCommCount) CommCount = nullptr;
        decltype(&ncclCommUserRank) CommUserRank = nullptr;
        decltype(&ncclAllGather) AllGather = nullptr;
        decltype(&ncclReduce) Reduce = nullptr;
        decltype(&ncclAllReduce) AllReduce = nullptr;
        decltype(&ncclGetErrorString) GetErrorString = nullptr;
        DevBuf<char> d_send, d_recv;
    } comm;
    std::string err;
    mibn_stats stats{}, total{};               // last call / since creation
    mibn_kernel_stat kstats[kStatSlots];  // per class (split_kinds) + the level kernel as a whole + the tiny kernel + the LDS-DMA sweep kernel
    mibn_kernel_stat ktotal[kStatSlots];  // + the device planner's pair of kernels + the concurrent launch pair of a level (option overlap)
                                          // + ve_max_kernel and mpe_traceback_kernel (mibn_mpe_batch: last-call statistics only)
    // the blocking, host-planned elimination calls (run_elim: mibn_mpe_batch, mibn_posterior_sample_batch): one set of buffers for
    // both - nothing a query call reads - beside the arena of lane 0
    struct Elim {
        std::vector<ProgBuf> bufs;  // malloc-backed program buffers, one per worker
        BatchPlan plan;
        Schedule sched;
        std::vector<LaunchGroup> groups;  // the launches of `sched`: one per level
        DevBuf<uint32_t> d_prog;
        DevBuf<uint64_t> d_prog_off, d_arena_off;
        DevBuf<Item> d_items;
        DevBuf<uint32_t> d_wg_item;
        DevBuf<double> d_m, d_log_p;  // per request of a chunk: what its FINAL step wrote; (MPE) the logarithm of it
        DevBuf<int32_t> d_codes;      // the decoded assignments of a chunk (MPE) / the rows of a draw launch
        DevBuf<DrawItem> d_draw_items;
        DevBuf<int64_t> d_m_off;      // (MAP) per request of a chunk: where its codes go in d_codes
        ChunkSeeds seeds;             // a call with likelihood findings
        std::vector<Event> ev;
        ~Elim() { for (ProgBuf &b : bufs) b.release(); }
    } elim;
    // mibn_expect_batch (blocking, host-planned): while `expect` is set, a query call hands its device-resident results to expect_run
    // instead of downloading them.  Buffers of its own; last-call statistics only (nothing a later query call reads).
    struct Expect {
        ExpectPlan plan;
        const double *weight = nullptr;
        int64_t B = 0, n_acc = 0;
        double *acc = nullptr, *p_out = nullptr;  // host
        DevBuf<char> d_meta;
        DevBuf<double> d_f64;  // [acc | p_out | weight | slab partials]
        Event ev[2];
    } ex;
    bool expect = false;
    // mibn_set_likelihoods: `staged` belongs to the next batch call, which takes it - `lh` points at it while that call runs - or refuses it;
    // either way it is gone when the call returns
    Findings staged;
    bool has_staged = false;
    const Findings *lh = nullptr;
    // mibn_dataset_create / mibn_score_families: code matrices resident on the device (id = index; a destroyed entry keeps its slot, so an
    // id is never handed out twice) and the buffers of a scoring call.  Nothing a query call reads; last-call statistics only.
    struct Dataset {
        DevBuf<uint8_t> d_codes;  // [n_cols][n_rows]
        int64_t n_rows = 0;
        int32_t n_cols = 0;
        std::vector<int32_t> card;
        bool live = false;
        // mibn_dataset_set_weights / mibn_dataset_bootstrap: the weight sets [n_sets][n_rows] and W_s of every set
        DevBuf<uint32_t> d_weights;
        int32_t n_sets = 0;
        std::vector<int64_t> weight_sum;
    };
    std::vector<Dataset> datasets;
    struct Score {
        DevBuf<unsigned long long> d_counts;
        DevBuf<char> d_meta;
        DevBuf<double> d_f64;  // [scores | partials of the chunked tables]
        DevBuf<long long> d_i64;  // mibn_ci_tests: the degrees of freedom, laid out as d_f64
        std::vector<Event> ev;
    } sc;
    int64_t score_cells = kScoreCellBudget;  // option score_cells (test hook: forces sub-batches)
    // mibn_best_dag and mibn_arc_posteriors (both blocking, on an idle context): the tables of a call (kept between calls up to
    // kDagKeepBytes), its candidate / result block and the events between its phases
    struct Dag {
        DevBuf<double> d_score, d_best;  // mibn_arc_posteriors: alpha / Gamma in d_score, L in d_best, R in d_right
        DevBuf<uint32_t> d_mask;
        DevBuf<uint8_t> d_sink;
        DevBuf<double> d_right;
        DevBuf<char> d_io;  // [fam_score | fam_child | fam_parents] then what the call carves behind them (DagFrame::carve)
        Event ev[5];
    } dag;
    int dag_tile_bits = kDagTileBits;    // options dag_tile_bits / dag_group_bits (test hooks: force multi-pass schedules at small n;
    int dag_group_bits = kDagGroupBits;  // no bit of mibn_best_dag depends on them, the last bits of mibn_arc_posteriors do: dag_plan.h says why)
    int weighted_share = 1;  // option weighted_share: count_weighted_kernel keeps a row's cell index across neighbouring tables of one scope (DESIGN section 24 has both times)
    // options
    double arena_gb = 200.0;  // scratch budget of all lanes together (of the 288 GB)
    int mfma_kernel = 1;            // round 5: the one-table fp64-MFMA pair classes of a level as a launch of ve_mfma_kernel (128 VGPRs, four
                                    // waves per SIMD) on a fourth stream instead of workgroups of ve_level_kernel (168 VGPRs, three): 296.2 -> 300.4 k queries/s,
                                    // all kernels 4.56 -> 4.63 TB/s, three interleaved repetitions each (profiles/r05_b_ab.log)
    int seg_kernel = 1;             // the segments of a level as a launch of ve_segment_kernel (12 KB of LDS per workgroup) instead of workgroups
                                    // of ve_level_kernel (40 KB, 168 VGPRs)
    Event epoch;                    // reference of the busy-time bookkeeping (re-recorded when the GPU is idle)
    Event lane_ev, zero_ev;         // end of lane 1's work of a call / results buffer zeroed
    double busy_until = 0;          // ms since epoch up to which GPU time has been booked as kernel_ms
    int n_streams = 1;  // lanes.  1 (default): every chunk on the main stream, one after the other.  2: consecutive chunks run concurrently
                        // (+3 % with 8 192-request chunks, profiles/r02_y_lanes*.log; the per-launch event times then include the other lane's
                        // contention and stop being a roofline measurement, which is why it is not the default)
    int first_chunk = 1;  // short first chunk of a call: 0 never, 1 when the GPU is idle, 2 always
    int threads = 0;
    int trace = 0;        // debug: one stderr line per launch
    int split_kinds = 0;  // profiling: one launch per (level, class of work) instead of one per level
    int overlap = 1;      // the sweep launch of a level goes to a second stream, beside the level kernel's launch of the same level (their
                          // items belong to different requests): the tail of one runs under the body of the other, +1-2 % (profiles/r03_k_overlap.log)
    int sweep_dma = 1;    // the sweep kernel: 1 = ve_sweep_dma_kernel (round 3: LDS-DMA fill, 16-byte LDS accesses, wave-local stage pairs,
                          // wave-owned tail); 0 = round 2's register-staged ve_sweep_kernel (reference for A/B runs and the bit-for-bit test)
    int gibbs_lds = 1;    // Gibbs: 1 = CPTs in LDS when they fit + the eight-lanes-per-chain form for grids (gibbs_kernel8); 2 = LDS, one chain per
                          // lane (round 3's kernel); 0 = always read the tables through L2
    int bp_lds = 1;       // mibn_bp_batch: 0 = the message arrays in slabs of the arena even where they fit in LDS (test hook, like gibbs_lds)
    int64_t chunk = 32768;  // requests per launch; planning of chunk i+1 overlaps the kernel of chunk i.  Round 3: 32 768 (16 384 before):
                            // half as many, twice as large launches - the tails of the ~150 launches of a chunk cost the same time
                            // whatever their size: 4.13-4.24 -> 4.30-4.38 TB/s over all kernels (profiles/r03_d_chunk.log); the
                            // arena of a C3 chunk doubles to ~145 GB of the 288
};

#define HIP_TRY(h, expr)                                                                              \
    do {                                                                                              \
        hipError_t e_ = (expr);                                                                       \
        if (e_ != hipSuccess) {                                                                       \
            (h)->err = std::string(#expr) + ": " + hipGetErrorString(e_);                             \
            return MIBN_E_HIP;                                                                        \
        }                                                                                             \
    } while (0)

// The arrays order_search.h reads, in one device buffer (rebuilt by set_network / set_order_hints).
static int upload_order_net(mibn_ctx *h) {
    h->order_net_ok = false;
    if (h->planner_only || h->net.n_vars > 128 || h->net.n_vars < 1) return MIBN_OK;
    const Network &net = h->net;
    const size_t n = (size_t)net.n_vars, nh = net.hint_sorted.size();
    std::vector<char> buf;
    auto put = [&](const void *p, size_t bytes) {
        const size_t off = (buf.size() + 15) & ~size_t(15);
        buf.resize(off + bytes);
        if (bytes) std::memcpy(buf.data() + off, p, bytes);
        return off;
    };
    const size_t o_card = put(net.card.data(), n * 4), o_depth = put(net.depth.data(), n * 4);
    const size_t o_asc = put(net.topo_asc.data(), n * 4), o_desc = put(net.topo_desc.data(), n * 4);
    const size_t o_hint = put(net.hint_flat.data(), nh * n * 4), o_log = put(net.log2card.data(), n * 8);
    const size_t o_anc = put(net.anc2.data(), n * sizeof(B2)), o_sc = put(net.scope2.data(), n * sizeof(B2));
    const size_t o_fam = put(net.fam2.data(), n * sizeof(B2));
    HIP_TRY(h, h->d_order_net.reset(buf.size()));
    HIP_TRY(h, hipMemcpy(h->d_order_net, buf.data(), buf.size(), hipMemcpyHostToDevice));
    OrderNet &o = h->order_net_dev;
    o = net.order_view();
    char *d = h->d_order_net;
    o.card = reinterpret_cast<const int32_t *>(d + o_card);
    o.depth = reinterpret_cast<const int32_t *>(d + o_depth);
    o.topo_asc = reinterpret_cast<const int32_t *>(d + o_asc);
    o.topo_desc = reinterpret_cast<const int32_t *>(d + o_desc);
    o.hint_sorted = reinterpret_cast<const int32_t *>(d + o_hint);
    o.log2card = reinterpret_cast<const double *>(d + o_log);
    o.anc = reinterpret_cast<const B2 *>(d + o_anc);
    o.cpt_scope = reinterpret_cast<const B2 *>(d + o_sc);
    o.fam = reinterpret_cast<const B2 *>(d + o_fam);
    h->order_net_ok = true;
    return MIBN_OK;
}

// The arrays emit_core.h reads, in one device buffer (rebuilt by set_network).  Networks the device order search covers only.
static int upload_emit_net(mibn_ctx *h) {
    h->emit_net_ok = false;
    if (h->planner_only || h->net.n_vars > 128 || h->net.n_vars < 1) return MIBN_OK;
    const Network &net = h->net;
    const size_t n = (size_t)net.n_vars;
    std::vector<char> buf;
    auto put = [&](const void *p, size_t bytes) {
        const size_t off = (buf.size() + 15) & ~size_t(15);
        buf.resize(off + bytes);
        if (bytes) std::memcpy(buf.data() + off, p, bytes);
        return off;
    };
    const size_t o_card = put(net.card.data(), n * 4), o_log = put(net.log2card.data(), n * 8), o_pool = put(net.pool_off.data(), n * 8);
    const size_t o_soff = put(net.scope_off32.data(), (n + 1) * 4), o_sv = put(net.scope_flat.data(), net.scope_flat.size() * 4);
    const size_t o_ss = put(net.cstride_flat.data(), net.cstride_flat.size() * 8), o_anc = put(net.anc_flat.data(), net.anc_flat.size() * 8);
    HIP_TRY(h, h->d_emit_net.reset(buf.size()));
    HIP_TRY(h, hipMemcpy(h->d_emit_net, buf.data(), buf.size(), hipMemcpyHostToDevice));
    EmitNet &e = h->emit_net_dev;
    e = net.emit_view();
    char *d = h->d_emit_net;
    e.card = reinterpret_cast<const int32_t *>(d + o_card);
    e.log2card = reinterpret_cast<const double *>(d + o_log);
    e.pool_off = reinterpret_cast<const int64_t *>(d + o_pool);
    e.scope_off = reinterpret_cast<const int32_t *>(d + o_soff);
    e.scope_vars = reinterpret_cast<const int32_t *>(d + o_sv);
    e.scope_stride = reinterpret_cast<const int64_t *>(d + o_ss);
    e.anc = reinterpret_cast<const uint64_t *>(d + o_anc);
    h->emit_net_ok = true;
    return MIBN_OK;
}

// The state an entry point needs, checked in this order: no asynchronous call in flight, a HIP device, a network.
enum : unsigned { kNeedIdle = 1, kNeedDevice = 2, kNeedNet = 4 };
static int check_state(mibn_ctx *h, unsigned need) {
    if ((need & kNeedIdle) && (h->pend[0].active || h->pend[1].active)) { h->err = "asynchronous calls in flight: collect them with mibn_wait first"; return MIBN_E_STATE; }
    if ((need & kNeedDevice) && h->planner_only) { h->err = "planner-only context: no HIP device bound (there is no CPU fallback)"; return MIBN_E_NODEVICE; }
    if ((need & kNeedNet) && !h->has_net) { h->err = "set_network first"; return MIBN_E_STATE; }
    return MIBN_OK;
}

extern "C" {

const char *mibn_version(void) { return "mibn 0.1 (gfx950)"; }

int mibn_device_count(int *count) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) n = 0;
    if (count) *count = n;
    return MIBN_OK;
}

// Factors of at most this many cells are "small" (segments, the small inputs of the passes, the byte model's big / small line).  1 024 from round 2 to the
// last day of round 6; with order_effort 1's plans 512 runs 1.3 % less GPU time per step (808.6 - 810.1 against 819.0 - 820.4 ms, interleaved; 256: 810.5; 2 048: 824.7 -
// profiles/r06_ca_ab.log, r06_cb_ab.log).  A bare Network (tools, oracle, the pinned fingerprints) keeps 1 024.
constexpr int kEngineSmallCells = 512;

int mibn_create_planner(mibn_t **out) {
    if (!out) return MIBN_E_ARG;
    auto *h = new mibn_ctx();
    h->net.order_effort = 1; h->net.second_above = h->pol.base_second_above;  // (the engine's default; a bare Network - the tools, the oracle - keeps round 5's search)
    h->net.small_cells = kEngineSmallCells;
    h->net.minfill_above = h->pol.base_minfill;
    h->planner_only = true;
    *out = h;
    return MIBN_OK;
}

int mibn_create(int device, mibn_t **out) {
    if (!out) return MIBN_E_ARG;
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return MIBN_E_NODEVICE;
    if (device < 0 || device >= n) return MIBN_E_ARG;
    auto *h = new mibn_ctx();
    h->net.order_effort = 1; h->net.second_above = h->pol.base_second_above;
    h->net.small_cells = kEngineSmallCells;
    h->net.minfill_above = h->pol.base_minfill;
    h->device = device;
    if (hipSetDevice(device) != hipSuccess) { delete h; return MIBN_E_NODEVICE; }
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) != hipSuccess) { delete h; return MIBN_E_NODEVICE; }
    if (std::string(prop.gcnArchName).rfind("gfx950", 0) != 0) {  // kernels are built for gfx950 only
        delete h;
        return MIBN_E_NODEVICE;
    }
    h->n_cu = prop.multiProcessorCount;
    bool ok = true;
    for (Stream *q : {&h->stream, &h->stream2, &h->aux[0][0], &h->aux[0][1], &h->aux[1][0], &h->aux[1][1], &h->aux[0][2], &h->aux[1][2], &h->copy_stream})
        ok = ok && q->ensure(hipStreamNonBlocking) == hipSuccess;
    // the sweep kernel keeps its 64 KiB tile, the T tables and the step descriptor in dynamic LDS (two workgroups per CU)
    ok = ok && hipFuncSetAttribute((const void *)ve_sweep_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, kSweepLdsBytes) == hipSuccess;
    ok = ok && hipFuncSetAttribute((const void *)ve_sweep_dma_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, kSweepLdsBytes) == hipSuccess;
    if (!ok) { delete h; return MIBN_E_HIP; }
    *out = h;
    return MIBN_OK;
}

void mibn_destroy(mibn_t *h) {
    if (!h) return;
    if (!h->planner_only) {
        (void)hipSetDevice(h->device);
        if (h->stream) (void)hipStreamSynchronize(h->stream);
        if (h->stream2) (void)hipStreamSynchronize(h->stream2);
        (void)mibn_comm_destroy(h);
    }
    delete h;  // (the members free what they own: buffers and events first, the streams last)
}

const char *mibn_last_error(const mibn_t *h) { return h ? h->err.c_str() : "null handle"; }

int mibn_set_option(mibn_t *h, const char *name, double value) {
    if (!h || !name) return MIBN_E_ARG;
    std::string n(name);
    if (n == "arena_gb") h->arena_gb = value;
    else if (n == "threads") h->threads = (int)value;
    else if (n == "chunk") h->chunk = std::max<int64_t>(1, (int64_t)value);
    else if (n == "big_iters") h->net.big_iters = std::max<int64_t>(1, (int64_t)value);  // test hooks: force tiling
    else if (n == "tile_h") h->net.tile_h = std::max(0, std::min(kTileMax, (int)value));  // 0 = sized by traffic
    else if (n == "tile_kb") h->net.tile_bytes = std::max<int64_t>(16, (int64_t)value) << 10;  // traffic per tile when tile_h = 0
    else if (n == "chunk_sets") { if (mibn_drain(h) != MIBN_OK) return MIBN_E_HIP; h->n_sets = std::max(2, std::min(kChunkSets, (int)value)); h->set_cursor = 0; }
    else if (n == "trace") h->trace = (int)value;
    else if (n == "split_kinds") h->split_kinds = value != 0;
    else if (n == "overlap") { if (mibn_drain(h) != MIBN_OK) return MIBN_E_HIP; h->overlap = value != 0; }
    else if (n == "sweep_dma") h->sweep_dma = value != 0;
    else if (n == "seg_kernel") h->seg_kernel = value != 0;
    else if (n == "gibbs_lds") h->gibbs_lds = std::max(0, std::min(2, (int)value));
    else if (n == "bp_lds") h->bp_lds = value != 0;
    else if (n == "tiny") h->tiny = value != 0;
    else if (n == "tiny_zero_copy") h->tiny_zero_copy = value != 0;
    else if (n == "mfma_kernel") h->mfma_kernel = value != 0;  // (round 6 measured CHAIN and OUTER in ve_mfma_kernel too: at its 128 registers they spill 74 and the
                                                                //  whole kernel pays - 291 against 298 k queries/s in three interleaved repetitions, profiles/r06_y_ab.log)
    else if (n == "gpu_emit") h->gpu_emit = std::max(0, std::min(2, (int)value));  // whole chunks planned on the device (order search + program emission)
    else if (n == "wave_wgs") h->wave_wgs = std::max(0, (int)value);
    else if (n == "plan_priority") h->plan_priority = std::max(0, std::min(2, (int)value));
    else if (n == "wave_plan") h->wave_plan = value != 0;  // 0: the device plans with order_kernel + emit_kernel (one request per lane)
    else if (n == "plan_waves") h->plan_waves = std::max(1, std::min(16, (int)value));  // waves per workgroup of the device planner's kernels
    else if (n == "plan_sort") h->plan_sort = (int)value;
    else if (n == "wave_sort") h->wave_sort = value != 0;  // wave_plan_kernel hands out the requests with the most relevant variables first (default 1)
    else if (n == "plan_lanes") h->plan_lanes = std::max(0, std::min(64, (int)value));  // requests per wave of the device planner's kernels
    else if (n == "emit_share") { h->pol.emit_share_opt = value > 0 ? std::min(1.0, value) : -1; if (value > 0) h->pol.emit_share = h->pol.emit_share_opt; }  // the device's share of a chunk (<= 0: follows the measured rates)
    else if (n == "emit_words") h->emit_words = (uint32_t)std::max(1024, std::min(1 << 20, (int)value));  // words of a request's device program slot
    else if (n == "gpu_search") h->gpu_search = std::max(0, std::min(2, (int)value));  // elimination-order search on the device
        // (order_kernel): 1 = the first chunk of a call on the host, the rest of the call by one launch; 2 = every chunk, synchronously (tests)
    else if (n == "adaptive") {
        h->pol.adaptive = value != 0;
        if (!h->pol.adaptive) {  // what the policy had switched goes back
            h->net.minfill_above = h->pol.base_minfill;
            if (h->pol.auto_emit) { h->gpu_emit = 0; h->pol.auto_emit = false; }
            if (h->pol.auto_search) { h->gpu_search = 0; h->pol.auto_search = false; }
            h->pol.adaptive_seeded = false;
        }
    }
    else if (n == "minfill_above") { h->pol.base_minfill = value; h->net.minfill_above = value; }  // bytes of the best sweep above which min-fill runs  // small-network kernel (one lane per request, no planning) where eligible
    else if (n == "fuse") h->net.fuse = value != 0;
    else if (n == "plan_cache") h->net.plan_cache = value != 0;  // plan templates for repeated request shapes
    else if (n == "chain") h->net.chain = value != 0;  // CHAIN form: three variables per pass
    else if (n == "streams") { if (mibn_drain(h) != MIBN_OK) return MIBN_E_HIP; h->n_streams = value >= 2 ? 2 : 1; h->n_sets = 2 * h->n_streams; h->set_cursor = 0; }  // lanes: 2 (default) = consecutive chunks run concurrently on two streams; 1 = one after the other
    else if (n == "first_chunk") h->first_chunk = std::max(0, std::min(2, (int)value));
    else if (n == "builtin_sweeps") {  // two depth-first topological orders as candidate elimination orders (rebuilds the hint lists)
        h->net.builtin_sweeps = value != 0;
        if (h->net.n_vars > 0) {
            std::vector<int32_t> flat;
            for (const auto &hh : h->net.hints) flat.insert(flat.end(), hh.begin(), hh.end());
            h->net.set_hints((int32_t)h->net.hints.size(), flat.data());
            if (!h->planner_only) return upload_order_net(h);
        }
    }
    else if (n == "order_effort") h->net.order_effort = std::max(0, std::min(1, (int)value));  // 1: more candidate orders, the byte model's best two both emitted where the best is expensive (order_search.h)
    else if (n == "second_above") { h->pol.base_second_above = value; h->net.second_above = value; }  // modelled bytes above which the runner-up order is emitted too
    else if (n == "second_on_device") h->second_on_device = value != 0;  // 1: also in the calls the device plans (default: those run without the second emission)
    else if (n == "order_weights") h->net.order_weights = std::max(0, std::min(64, (int)value));  // class-weighted byte model of the order search (0: plain section-8(d) bytes)
    else if (n == "sweep_canon") h->net.sweep_canon = value != 0;  // test hook: 0 = the sweep kernel's general path for every step
    else if (n == "sweep_adapt") h->net.sweep_adapt = std::max(0, (int)value);  // fewer tiles per workgroup in sweep launches below this many workgroups
    else if (n == "sweep_min") h->net.sweep_min = std::max(2, std::min(5, (int)value));  // fewest variables of a SWEEP pass
    else if (n == "sweep_iters") h->net.sweep_iters = std::max(1, std::min(kTileMax, (int)value));  // tiles per workgroup of the sweep kernel
    else if (n == "sweep") h->net.sweep = std::max(0, std::min(5, (int)value));  // SWEEP form: up to this many variables per pass, tile in LDS (0 / < 3: off)
    else if (n == "outer") h->net.outer = value != 0;
    else if (n == "stagger") h->net.stagger = std::max(1, std::min(8, (int)value));  // groups of requests with staggered levels per chunk
    else if (n == "prune") h->net.prune = value != 0;  // 0: multiply every CPT (full_joint_dist / predict_proba semantics)  // OUTER (MFMA) form for products of two big tables  // joint elimination of two variables per pass
    else if (n == "weighted_share") h->weighted_share = value != 0;
    else if (n == "dag_tile_bits") h->dag_tile_bits = dag_clamp_bits((int64_t)value);
    else if (n == "dag_group_bits") h->dag_group_bits = dag_clamp_bits((int64_t)value);
    else if (n == "score_cells") h->score_cells = std::max<int64_t>(1, std::min<int64_t>(int64_t(1) << 28, (int64_t)value));  // test hook: cell budget of a sub-batch of mibn_score_families (2^28: at most 32 768 LDS groups, the grid's y limit is 65 535)
    else if (n == "small_cells") h->net.small_cells = std::max(1, std::min(kMaxT, (int)value));  // test hook: forces FIBER steps on small networks
    else { h->err = "unknown option " + n; return MIBN_E_ARG; }
    return MIBN_OK;
}

int mibn_set_network(mibn_t *h, int32_t n_vars, const int32_t *card, const int64_t *scope_off,
                     const int32_t *scope_vars, const int64_t *value_off, const double *values) {
    if (!h || !card || !scope_off || !scope_vars || !value_off || !values) return MIBN_E_ARG;
    std::string e = h->net.set(n_vars, card, scope_off, scope_vars, value_off, values);
    if (!e.empty()) { h->err = e; h->has_net = false; return MIBN_E_ARG; }
    h->has_net = true;
    h->pol.adaptive_seeded = false;  // (the adaptive policy starts over with a new network)
    if (h->pol.auto_emit) { h->gpu_emit = 0; h->pol.auto_emit = false; }
    if (!h->planner_only) {
        HIP_TRY(h, hipSetDevice(h->device));
        HIP_TRY(h, h->d_pool.reset(std::max<size_t>(1, h->net.pool.size())));
        HIP_TRY(h, hipMemcpy(h->d_pool, h->net.pool.data(), h->net.pool.size() * sizeof(double), hipMemcpyHostToDevice));
        h->tiny_ok = tiny_eligible(h->net);
        HIP_TRY(h, h->d_tiny_meta.release());
        if (h->tiny_ok) {
            const std::vector<int32_t> meta = tiny_meta(h->net);
            h->tiny_meta_words = (int32_t)meta.size();
            HIP_TRY(h, h->d_tiny_meta.reset(meta.size()));
            HIP_TRY(h, hipMemcpy(h->d_tiny_meta, meta.data(), meta.size() * 4, hipMemcpyHostToDevice));
            h->tiny_ok = tiny_lds_bytes((int)h->net.pool.size(), h->tiny_meta_words) <= 64 * 1024;
        }
        if (int rc = upload_emit_net(h)) return rc;
        return upload_order_net(h);
    }
    return MIBN_OK;
}

int mibn_set_order_hints(mibn_t *h, int32_t n_hints, const int32_t *priorities) {
    if (!h || n_hints < 0 || (n_hints && !priorities)) return MIBN_E_ARG;
    if (int rc = check_state(h, kNeedNet)) return rc;
    h->net.set_hints(n_hints, priorities);
    if (!h->planner_only) return upload_order_net(h);
    return MIBN_OK;
}

int mibn_last_stats(const mibn_t *h, mibn_stats *out) {
    if (!h || !out) return MIBN_E_ARG;
    *out = h->stats;
    return MIBN_OK;
}

int mibn_plan_stats(mibn_t *h, int32_t n_q, const int32_t *q_vars, int32_t n_e, const int32_t *e_vars,
                    mibn_stats *out) {
    if (!h || !out) return MIBN_E_ARG;
    if (int rc = check_state(h, kNeedNet)) return rc;
    Request rq;
    rq.nq = n_q; rq.qvars = q_vars; rq.ne = n_e; rq.evars = e_vars;
    std::string e = validate_request(h->net, rq);
    if (!e.empty()) { h->err = e; return MIBN_E_ARG; }
    std::vector<uint32_t> prog;
    PlanStats st;
    e = plan_request(h->net, rq, prog, st);
    if (!e.empty()) { h->err = e; return MIBN_E_LIMIT; }
    std::memset(out, 0, sizeof(*out));
    out->alg_bytes = st.alg_bytes;
    out->alg_flops = st.alg_flops;
    out->n_steps = st.n_steps;
    out->max_step_cells = st.max_step_cells;
    out->arena_bytes = 8.0 * (double)st.arena_cells;
    return MIBN_OK;
}

}  // extern "C"

namespace {

template <class T>
int ensure(mibn_ctx *h, DevBuf<T> &buf, size_t need) {
    HIP_TRY(h, buf.ensure(need));
    return MIBN_OK;
}

// pinned backing of the program buffers: the upload is then a real async DMA that overlaps planning
uint32_t *pinned_grow(void *, uint32_t *old, size_t used, size_t new_cap) {
    PinnedBuf fresh;
    if (fresh.reset(new_cap * sizeof(uint32_t)) != hipSuccess) return nullptr;
    if (old) {
        std::memcpy(fresh.get(), old, used * sizeof(uint32_t));
        (void)PinnedBuf::adopt(old).release();
    }
    return reinterpret_cast<uint32_t *>(fresh.detach());
}

// a pinned staging buffer of at least `bytes` (a quarter of headroom; what it held is not kept)
int pinned(mibn_ctx *h, PinnedBuf &sg, size_t bytes) {
    HIP_TRY(h, sg.ensure(bytes));
    return MIBN_OK;
}

// async upload through a pinned staging buffer (one per destination and set: reused only after retire())
int upload(mibn_ctx *h, PinnedBuf &sg, void *dst, const void *src, size_t bytes) {
    if (!bytes) return MIBN_OK;
    if (int rc = pinned(h, sg, bytes)) return rc;
    std::memcpy(sg.get(), src, bytes);
    HIP_TRY(h, hipMemcpyAsync(dst, sg.get(), bytes, hipMemcpyHostToDevice, h->copy_stream));
    return MIBN_OK;
}

// CPUs this process may actually use: the cgroup CPU quota when there is one (a container that sees 256 hardware
// threads may be limited to 16 CPUs' worth of time; more runnable threads than ~2x the quota only get throttled)
double cpu_quota() {
    double q = 0;
    if (FILE *f = std::fopen("/sys/fs/cgroup/cpu.max", "r")) {  // cgroup v2: "<quota|max> <period>"
        char a[64] = {0};
        double period = 0;
        if (std::fscanf(f, "%63s %lf", a, &period) == 2 && std::strcmp(a, "max") != 0 && period > 0) q = std::atof(a) / period;
        std::fclose(f);
    } else if (FILE *g = std::fopen("/sys/fs/cgroup/cpu/cpu.cfs_quota_us", "r")) {  // cgroup v1
        double quota = 0, period = 0;
        if (std::fscanf(g, "%lf", &quota) == 1 && quota > 0) {
            if (FILE *p = std::fopen("/sys/fs/cgroup/cpu/cpu.cfs_period_us", "r")) {
                if (std::fscanf(p, "%lf", &period) == 1 && period > 0) q = quota / period;
                std::fclose(p);
            }
        }
        std::fclose(g);
    }
    return q;
}

int default_threads() {
    int hw = (int)std::thread::hardware_concurrency();
    int local_world = 1;
    if (const char *e = std::getenv("LOCAL_WORLD_SIZE")) local_world = std::max(1, std::atoi(e));
    double cpus = hw;
    const double quota = cpu_quota();
    if (quota > 0) cpus = std::min(cpus, 2.0 * quota);  // planning is bursty: 2 threads per quota CPU finish a chunk sooner inside the same
                                                        // CPU-time budget; 4 per CPU (round 1's choice) run into the cgroup's throttling now that
                                                        // a step is 135 ms instead of 170 (profiles/r02_y_threads.log: 16-32 threads 237-239 k
                                                        // queries/s, 64 threads 235 k, 128 threads 221 k with 44 thread-seconds throttled)
    return std::max(1, std::min(64, (int)(cpus / local_world)));
}

void ensure_pool(mibn_ctx *h) {
    if (h->pool) return;
    h->pool.reset(new ThreadPool(h->threads > 0 ? h->threads : default_threads()));
    for (auto &st : h->set) {
        st.bufs.resize(h->pool->size());
        st.xbufs.resize(h->pool->size());
        if (!h->planner_only) {
            for (auto &b : st.bufs) b.grow = pinned_grow;
            for (auto &b : st.xbufs) b.grow = pinned_grow;
        }
    }
}

// name of statistics slot k: the classes of work (split_kinds), then the kernels as launched
const char *stat_name(int k) { return k < kNumKernels ? kernel_name(k) : kStatSlotNames[k - kNumKernels]; }

// adds to statistics slot `slot`: of the last call (`last`) and / or of the totals (`total`)
void book_stat(mibn_ctx *h, int slot, double launches, double ms, double bytes, double items, bool last, bool total) {
    for (mibn_kernel_stat *ks : {last ? &h->kstats[slot] : nullptr, total ? &h->ktotal[slot] : nullptr}) {
        if (!ks) continue;
        if (!ks->name[0]) std::snprintf(ks->name, sizeof(ks->name), "%s", stat_name(slot));
        ks->launches += launches;
        ks->ms += ms;
        ks->alg_bytes += bytes;
        ks->items += items;
    }
}

// every call that reports last-call statistics starts from zeroed, named slots
void reset_last_stats(mibn_ctx *h) {
    h->stats = mibn_stats{};
    for (int k = 0; k < kStatSlots; ++k) {
        h->kstats[k] = mibn_kernel_stat{};
        std::snprintf(h->kstats[k].name, sizeof(h->kstats[k].name), "%s", stat_name(k));
    }
}

// Wait for everything on the context's streams (search, copy, main, lane 1, the overlap streams): wait(q) for each, up to the first
// that fails.
template <class Wait>
int each_stream(mibn_ctx *h, Wait &&wait) {
    for (hipStream_t q : {h->search_stream.get(), h->copy_stream.get(), h->stream.get(), h->stream2.get()})
        if (q)
            if (int rc = wait(q)) return rc;
    for (auto &la : h->aux)
        for (const Stream &a : la)
            if (a)
                if (int rc = wait(a.get())) return rc;
    return MIBN_OK;
}
int drain_streams(mibn_ctx *h) {
    return each_stream(h, [h](hipStream_t q) -> int { HIP_TRY(h, hipStreamSynchronize(q)); return MIBN_OK; });
}
// error paths: every stream is waited for whatever it returns, and the error the call already has is the one reported
void drain_streams_unchecked(mibn_ctx *h) {
    (void)each_stream(h, [](hipStream_t q) -> int { (void)hipStreamSynchronize(q); return MIBN_OK; });
}
void drain_main_unchecked(mibn_ctx *h) {  // (the blocking elimination calls: all their work is on the main stream)
    if (h->stream) (void)hipStreamSynchronize(h->stream);
}

// Every error exit of a call drains what the call (and, with drain_streams_unchecked, earlier asynchronous calls) already put on the
// streams before the caller sees the error: the caller may free or reuse its request arrays and the pinned `out` the kernels and
// copies still touch (ADVICE r3 did this for the device-planner exits only; ADVICE r4: every exit behind the first launch).
int drained_on_error(mibn_ctx *h, int rc, void (*drain)(mibn_ctx *)) {
    if (rc != MIBN_OK && h && !h->planner_only) {
        const std::string keep = h->err;
        (void)hipSetDevice(h->device);
        drain(h);
        (void)hipGetLastError();
        h->err = keep;
    }
    return rc;
}

// wait for a set's launches and book their HIP-event durations per kernel
int retire(mibn_ctx *h, mibn_ctx::Set &st) {
    using Timed = mibn_ctx::Set::Timed;
    if (!st.busy) return MIBN_OK;
    HIP_TRY(h, hipEventSynchronize(st.ev[st.ev_used - 1]));
    for (auto &t : st.timed) {
        float ms = 0;
        if (t.kid != Timed::kLevelGroup) HIP_TRY(h, hipEventElapsedTime(&ms, st.ev[t.e[0][0]], st.ev[t.e[0][1]]));  // (a level's launch group: any of its event pairs may be absent)
        const bool mine = t.call == h->call_id;  // (launches of an earlier asynchronous call only count in the totals)
        if (t.kid == Timed::kWave) {
            h->retired_requests += t.items;  // (the wave's requests)
            // GPU time of a wave, first launch to last.  With two lanes the waves of consecutive chunks overlap: what is
            // booked as kernel_ms is the time the GPU was busy (the union of the intervals, kept as a high-water mark
            // since the epoch event; sets retire in launch order)
            float t0 = 0, t1 = 0;
            HIP_TRY(h, hipEventElapsedTime(&t0, h->epoch, st.ev[t.e[0][0]]));
            HIP_TRY(h, hipEventElapsedTime(&t1, h->epoch, st.ev[t.e[0][1]]));
            const double add = std::max(0.0, (double)t1 - std::max((double)t0, h->busy_until));
            h->busy_until = std::max(h->busy_until, (double)t1);
            if (mine) h->stats.kernel_ms += add;
            h->total.kernel_ms += add;
            continue;
        }
        if (t.kid == Timed::kLevelGroup) {
            // one level = one concurrent launch group: from the earliest start to the latest end (timestamps against the epoch event)
            double lo = 1e300, hi = -1e300;
            for (const auto &p : t.e)
                if (p[0] != Timed::kNone) { float x = 0; HIP_TRY(h, hipEventElapsedTime(&x, h->epoch, st.ev[p[0]])); lo = std::min(lo, (double)x); }
            for (const auto &p : t.e)
                if (p[1] != Timed::kNone) { float x = 0; HIP_TRY(h, hipEventElapsedTime(&x, h->epoch, st.ev[p[1]])); hi = std::max(hi, (double)x); }
            book_stat(h, kStatLevelGroup, 1, std::max(0.0, hi - lo), t.bytes, t.items, mine, true);
            continue;
        }
        if (mine) h->stats.n_launches += 1;
        h->total.n_launches += 1;
        book_stat(h, t.kid, 1, ms, t.bytes, t.items, mine, true);
        if (h->trace) std::fprintf(stderr, "[mibn launch] %-32s wgs %8.0f MB %10.2f ms %8.4f -> %7.1f GB/s\n", h->kstats[t.kid].name, t.items, t.bytes / 1e6, ms, t.bytes / ms / 1e6);
    }
    if (h->trace && st.gap_from >= 0 && st.ev_used > 0) {
        float gap = 0;
        if (hipEventElapsedTime(&gap, h->gap_ev[st.gap_from], st.ev[0]) == hipSuccess)
            std::fprintf(stderr, "[mibn gap] %.3f ms between the end of the previous wave and the first launch of this one\n", gap);
        st.gap_from = -1;
    }
    st.timed.clear();
    st.ev_used = 0;
    st.busy = false;
    return MIBN_OK;
}

// every set, oldest launches first (set_cursor points at the set that is re-used next = the oldest): the busy-time
// bookkeeping of retire() wants the waves in launch order
int retire_all(mibn_ctx *h) {
    for (int i = 0; i < h->n_sets; ++i) {
        int rc = retire(h, h->set[(h->set_cursor + i) % h->n_sets]);
        if (rc) return rc;
    }
    for (auto &st : h->set) {  // (sets beyond n_sets: idle unless the option has just changed)
        int rc = retire(h, st);
        if (rc) return rc;
    }
    return MIBN_OK;
}

int next_event(mibn_ctx *h, mibn_ctx::Set &st, size_t &idx, hipStream_t stream = nullptr) {
    if (st.ev_used == st.ev.size()) st.ev.emplace_back();
    idx = st.ev_used++;
    HIP_TRY(h, st.ev[idx].ensure());
    HIP_TRY(h, hipEventRecord(st.ev[idx], stream ? stream : h->stream));
    return MIBN_OK;
}

}  // namespace

namespace {
// Requests per wave of the device planner's kernels.  The lanes of a wave run different requests, every data-dependent branch
// diverges, so a wave's time grows with its lanes in use: fewer lanes in more waves plan faster and take more of the chip from the
// VE kernels.  A rank of one or two planning threads is bound by its planning capacity (host + device), not by its kernels: 24
// lanes (230 -> 246 k queries/s at one and two threads); from four threads on the kernels' share of the chip counts for more: 32
// (258 / 254 k at 24 / 32 lanes and four threads, 263 / 269 k at six; profiles/r05_f_planlanes.log, r05_g_planlanes.log).
// (Calls of 32 768 requests - such a rank's shard of a 2^18-request step on eight GPUs - are bound by the kernels again, whatever the lanes:
//  250.3 / 251.5 k at 24 / 32 lanes and two threads, 240 / 250 k at one: 32 there.  profiles/r05_k_calls32k.log)
// chunks the device plans go through wave_plan_kernel (its time grows with the requests it is given - order_kernel / emit_kernel are
// latency-bound: theirs hardly does): the host's share of a chunk may shrink to a hundredth
static bool wave_mode(const mibn_ctx *h) { return h->wave_plan && h->wnet_ok; }

// The planning stream, created on first use with the priority of option plan_priority.
static int plan_stream(mibn_ctx *h) {
    if (h->search_stream) return MIBN_OK;
    int lo = 0, hi = 0;
    HIP_TRY(h, hipDeviceGetStreamPriorityRange(&lo, &hi));
    HIP_TRY(h, h->search_stream.ensure(hipStreamNonBlocking, h->plan_priority >= 2 ? hi : (h->plan_priority == 1 ? (lo + hi) / 2 : lo)));
    return MIBN_OK;
}

static int plan_lanes_now(const mibn_ctx *h) {
    if (h->plan_lanes > 0) return h->plan_lanes;
    return h->pool && h->pool->size() <= 2 && h->chunk > 32768 ? 24 : 32;
}

// Device order search for requests [b0, b1): uploads their query / evidence variables and launches order_kernel on a
// high-priority stream of its own (it must not queue behind the level kernels of the previous chunk); the orders (128
// bytes per request) and their lengths land in h->search_out.  Asynchronous: search_wait() before they are read.  The
// kernel is latency-bound with one request per lane - its duration hardly depends on the number of requests - so the
// whole remainder of a call is searched by one launch (slices of kSearchSlice requests share the scratch buffer).
constexpr int64_t kSearchSlice = 65536;  // 1.3 GB of search state
int search_orders_async(mibn_ctx *h, uint32_t flags, int64_t b0, int64_t b1, const int64_t *q_off, const int32_t *q_vars,
                        const int64_t *e_off, const int32_t *e_vars) {
    const int64_t n = b1 - b0;
    int rc;
    if ((rc = plan_stream(h))) return rc;
    const size_t nq = (size_t)(q_off[b1] - q_off[b0]), ne = (size_t)(e_off[b1] - e_off[b0]);
    const size_t off_bytes = (size_t)(n + 1) * 8;
    const size_t in_bytes = 2 * off_bytes + (nq + ne) * 4 + 64;
    if ((rc = pinned(h, h->search_in, in_bytes))) return rc;
    if ((rc = pinned(h, h->search_out, (size_t)n * 132))) return rc;
    if ((rc = ensure(h, h->d_order_scratch, (size_t)std::min(n, kSearchSlice)))) return rc;
    int64_t *qo = reinterpret_cast<int64_t *>(h->search_in.get()), *eo = qo + (n + 1);
    for (int64_t i = 0; i <= n; ++i) { qo[i] = q_off[b0 + i] - q_off[b0]; eo[i] = e_off[b0 + i] - e_off[b0]; }
    char *pv = h->search_in.get() + 2 * off_bytes;
    std::memcpy(pv, q_vars + q_off[b0], nq * 4);
    if (ne) std::memcpy(pv + nq * 4, e_vars + e_off[b0], ne * 4);
    // (no copies on this stream - the kernel reads the request arrays from, and writes the orders to, pinned host memory: a DMA
    // copy here queues behind the previous call's result download on the copy engine, i.e. behind that call's kernels)
    const char *d_req = h->search_in.get();
    uint8_t *orders_out = reinterpret_cast<uint8_t *>(h->search_out.get());
    int32_t *len_out = reinterpret_cast<int32_t *>(h->search_out.get() + (size_t)n * 128);
    for (int64_t s0 = 0; s0 < n; s0 += kSearchSlice) {
        const int64_t m = std::min(kSearchSlice, n - s0);
        OrderArgs A;
        A.net = h->order_net_dev;
        A.net.prune = h->net.prune;
        A.net.minfill_above = h->net.minfill_above;
        {   // (options set after the network: the model weights follow them like on the host)
            const OrderNet hv = h->net.order_view();
            A.net.chain_weight = hv.chain_weight;
            A.net.big_cells = hv.big_cells;
            A.net.effort = hv.effort;
        }
        A.q_off = reinterpret_cast<const int64_t *>(d_req) + s0;
        A.e_off = reinterpret_cast<const int64_t *>(d_req + off_bytes) + s0;
        A.q_vars = reinterpret_cast<const int32_t *>(d_req + 2 * off_bytes);
        A.e_vars = A.q_vars + nq;
        A.B = m;
        A.flags = flags;
        A.orders = orders_out + s0 * 128;
        A.order_len = len_out + s0;
        A.scratch = h->d_order_scratch;
        A.zero = nullptr;
        A.perm = nullptr;
        A.lanes = plan_lanes_now(h);
        {
            const int64_t per_wg = (int64_t)A.lanes * h->plan_waves;
            hipLaunchKernelGGL(order_kernel, dim3((unsigned)((m + per_wg - 1) / per_wg)), dim3(64 * h->plan_waves), 0, h->search_stream, A);
        }
        HIP_TRY(h, hipGetLastError());
    }
    return MIBN_OK;
}

int search_wait(mibn_ctx *h) {
    HIP_TRY(h, hipStreamSynchronize(h->search_stream));
    return MIBN_OK;
}

// Device planning of requests [b0, b1) - one chunk - into set `st`: order_kernel, then emit_kernel, on the planning stream (high
// priority: its few waves must not queue behind the level kernels of the chunk in flight); the programs stay on the device
// (st.d_prog, one slot of h->emit_words words per request), the per-request results and the work items come back and fill
// the BatchPlan like plan_batch would.  Returns MIBN_OK, an error, or 1: a request did not fit its slot / the item buffer
// (the caller plans the chunk on the host; the slots double for the next chunk).
constexpr int64_t kPlanSlice = 32768;  // requests per launch pair: 1.1 GB of search state + ~8 GB of emission state (100 variables)
int plan_on_device_launch(mibn_ctx *h, uint32_t flags, int64_t b0, int64_t b1, const int64_t *q_off, const int32_t *q_vars, const int64_t *e_off,
                          const int32_t *e_vars, const int32_t *e_codes, const int64_t *out_off, const char *skip, mibn_ctx::Set &st, size_t prog_words) {
    const int64_t n = b1 - b0;
    int rc;
    if ((rc = plan_stream(h))) return rc;
    hipStream_t P = h->search_stream;
    const size_t nq = (size_t)(q_off[b1] - q_off[b0]), ne = (size_t)(e_off[b1] - e_off[b0]);
    const size_t off_bytes = (size_t)(n + 1) * 8;
    const size_t perm_off = (3 * off_bytes + (nq + 2 * ne) * 4 + (size_t)n + 63) & ~(size_t)63;
    const size_t in_bytes = perm_off + (size_t)n * 4 + 64;
    const size_t stride = h->emit_words;
    const size_t tag_cap = (size_t)n * 64;
    const size_t scratch_stride = emit_scratch_bytes(h->net.n_vars);
    const int64_t slice = std::min(n, kPlanSlice);
    // the wave-cooperative planner (wave_plan_kernel) where the network and the options of the moment are covered: its packed copy of
    // them is rebuilt per chunk (10 KB) and uploaded when it has changed
    bool wave = false;
    if (h->wave_plan && h->order_net_ok) {
        if (!h->wnet_host) { h->wnet_host.reset(new WNet); std::memset(h->wnet_host.get(), 0, sizeof(WNet)); h->wnet_ok = false; }
        std::unique_ptr<WNet> fresh(new WNet);
        if (h->net.wave_view(*fresh)) {
            if (!h->d_wnet) HIP_TRY(h, h->d_wnet.reset(1));
            if (!h->wnet_ok || std::memcmp(fresh.get(), h->wnet_host.get(), sizeof(WNet)) != 0) {
                HIP_TRY(h, hipMemcpy(h->d_wnet, fresh.get(), sizeof(WNet), hipMemcpyHostToDevice));
                std::memcpy(h->wnet_host.get(), fresh.get(), sizeof(WNet));
                h->wnet_ok = true;
            }
            wave = true;
        }
    }
    if ((rc = pinned(h, h->emit_in, in_bytes))) return rc;
    if ((rc = pinned(h, h->emit_out, (size_t)n * sizeof(EmitMeta) + tag_cap * sizeof(Tag) + 64))) return rc;
    if (!h->d_emit_cursor) HIP_TRY(h, h->d_emit_cursor.reset(16));  // (64 bytes)
    if (!wave) {
    if ((rc = ensure(h, h->d_orders, (size_t)n * 128))) return rc;
    if ((rc = ensure(h, h->d_order_len, (size_t)n))) return rc;
    if ((rc = ensure(h, h->d_order_scratch, (size_t)slice))) return rc;
    }
    if (!wave && (size_t)slice * scratch_stride > h->d_emit_scratch.cap())
        HIP_TRY(h, h->d_emit_scratch.reset((size_t)std::max<int64_t>(slice, std::min<int64_t>(h->chunk, kPlanSlice)) * scratch_stride));
    if ((rc = ensure(h, st.d_prog, std::max(prog_words, (size_t)n * stride) + kMaxStepWords))) return rc;  // (slack: segment_wave prefetches whole descriptor slots)  // (+ room for the host's share of the chunk)
    HIP_TRY(h, h->emit_ev[0].ensure());
    HIP_TRY(h, h->emit_ev[1].ensure());
    // the request arrays of the chunk in one pinned buffer: [q_off | e_off | out_off | q_vars | e_vars | e_codes | skip]
    char *pin = h->emit_in.get();
    int64_t *qo = reinterpret_cast<int64_t *>(pin), *eo = qo + (n + 1), *oo = eo + (n + 1);
    for (int64_t i = 0; i <= n; ++i) { qo[i] = q_off[b0 + i] - q_off[b0]; eo[i] = e_off[b0 + i] - e_off[b0]; oo[i] = out_off[b0 + i] - out_off[b0]; }
    char *pv = pin + 3 * off_bytes;
    std::memcpy(pv, q_vars + q_off[b0], nq * 4);
    if (ne) { std::memcpy(pv + nq * 4, e_vars + e_off[b0], ne * 4); std::memcpy(pv + (nq + ne) * 4, e_codes + e_off[b0], ne * 4); }
    std::memcpy(pv + (nq + 2 * ne) * 4, skip + b0, (size_t)n);
    // lane position -> request, slice by slice: descending size of the relevant set (query, evidence and their ancestors: what the order
    // search and the emission loop over), a counting sort on 129 keys
    int32_t *perm = reinterpret_cast<int32_t *>(pin + perm_off);
    const bool sorted = h->plan_sort && h->net.n_vars <= 128 && !h->net.anc2.empty();
    if (sorted) {
        std::vector<uint8_t> key((size_t)std::min(n, kPlanSlice));
        for (int64_t s0 = 0; s0 < n; s0 += kPlanSlice) {
            const int64_t m = std::min(kPlanSlice, n - s0);
            int32_t count[130] = {0};
            for (int64_t i = 0; i < m; ++i) {
                const int64_t b = b0 + s0 + i;
                B2 rel;
                for (int64_t k = q_off[b]; k < q_off[b + 1]; ++k) { const int v = q_vars[k]; rel.set(v); rel.a |= h->net.anc2[v].a; rel.b |= h->net.anc2[v].b; }
                for (int64_t k = e_off[b]; k < e_off[b + 1]; ++k) { const int v = e_vars[k]; rel.set(v); rel.a |= h->net.anc2[v].a; rel.b |= h->net.anc2[v].b; }
                const int c = 128 - b2_count(rel);  // (descending)
                key[(size_t)i] = (uint8_t)c;
                ++count[c + 1];
            }
            for (int c = 0; c < 129; ++c) count[c + 1] += count[c];
            if (h->plan_sort == 1) {
                for (int64_t i = 0; i < m; ++i) perm[s0 + count[key[(size_t)i]]++] = (int32_t)i;
            } else {
                // plan_sort = 2: the sorted requests dealt round-robin over the workgroups - every workgroup (= CU) gets the same mix of
                // sizes, and inside it the waves are homogeneous (rank r -> workgroup r mod G, slot r div G)
                // (plan_sort = 3: the same over the WAVES - rank r -> wave r mod W: every wave gets the same sum of sizes, what counts if the
                //  lanes of a wave serialise)
                const int64_t per = h->plan_sort == 3 ? (int64_t)plan_lanes_now(h) : (int64_t)plan_lanes_now(h) * h->plan_waves, G = (m + per - 1) / per;
                std::vector<int32_t> rank_of((size_t)m);
                for (int64_t i = 0; i < m; ++i) rank_of[(size_t)count[key[(size_t)i]]++] = (int32_t)i;  // rank -> request
                std::vector<int64_t> fill((size_t)G, 0);
                // (the last workgroup may be short: a slot beyond the slice is skipped by giving the rank to the next workgroup with room)
                int64_t g = 0;
                for (int64_t r = 0; r < m; ++r) {
                    for (int tries = 0; tries < G; ++tries, g = (g + 1) % G) {
                        const int64_t pos = g * per + fill[(size_t)g];
                        if (fill[(size_t)g] < per && pos < m) { perm[s0 + pos] = rank_of[(size_t)r]; ++fill[(size_t)g]; g = (g + 1) % G; break; }
                    }
                }
            }
        }
    }
    // No copies on the planning stream: its kernels read the request arrays from, and write their results to, pinned host
    // memory.  (A DMA copy on this stream queued behind the previous call's result download - which waits for that call's
    // kernels - on the copy engine: the planner started when the chunk in flight had finished, never beside it.)
    HIP_TRY(h, hipEventRecord(h->emit_ev[0], P));
    const char *d = pin;
    EmitMeta *meta_out = reinterpret_cast<EmitMeta *>(h->emit_out.get());
    Tag *tags_out = reinterpret_cast<Tag *>(h->emit_out.get() + (size_t)n * sizeof(EmitMeta) + 64);
    if (wave) {
        WavePlanArgs A;
        A.net = h->d_wnet;
        A.anc = h->order_net_dev.anc;
        A.q_off = reinterpret_cast<const int64_t *>(d);
        A.e_off = reinterpret_cast<const int64_t *>(d + off_bytes);
        A.out_off = reinterpret_cast<const int64_t *>(d + 2 * off_bytes);
        A.q_vars = reinterpret_cast<const int32_t *>(d + 3 * off_bytes);
        A.e_vars = A.q_vars + nq;
        A.e_codes = A.e_vars + ne;
        A.skip = reinterpret_cast<const char *>(A.e_codes + ne);
        A.B = n;
        A.flags = flags;
        A.prog = st.d_prog;
        A.prog_stride = (uint32_t)stride;
        A.meta = meta_out;
        A.tags = tags_out;
        A.tag_cursor = h->d_emit_cursor;
        A.tag_cap = (uint32_t)tag_cap;
        A.perm = nullptr;
        if (h->wave_sort && n > 4 * kWaveWG * (int64_t)h->n_cu) {  // (fewer requests than waves in flight: nothing to order)
            if ((rc = ensure(h, h->d_plan_perm, 2 * (size_t)n))) return rc;
            A.perm = h->d_plan_perm;
        }
        hipLaunchKernelGGL(reset_cursor_kernel, dim3(1), dim3(1), 0, P, h->d_emit_cursor);
        if (A.perm) hipLaunchKernelGGL(plan_sort_kernel, dim3(1), dim3(kPlanSortThreads), 0, P, A);
        {
            // (the waves draw requests from a counter: the grid is what the chip holds at once - MIBN_WAVE_MIN_WGS workgroups per CU)
            int64_t grid = std::min<int64_t>((n + kWaveWG - 1) / kWaveWG, (int64_t)h->n_cu * MIBN_WAVE_MIN_WGS);
            if (h->wave_wgs > 0) grid = std::min<int64_t>(grid, h->wave_wgs);
            hipLaunchKernelGGL(wave_plan_kernel, dim3((unsigned)grid), dim3(64 * kWaveWG), 0, P, A);
        }
        HIP_TRY(h, hipGetLastError());
    }
    for (int64_t s0 = 0; !wave && s0 < n; s0 += kPlanSlice) {
        const int64_t m = std::min(kPlanSlice, n - s0);
        OrderArgs O;
        O.net = h->order_net_dev;
        O.net.prune = h->net.prune;
        O.net.minfill_above = h->net.minfill_above;
        {   // (options set after the network: the model weights follow them like on the host)
            const OrderNet hv = h->net.order_view();
            O.net.chain_weight = hv.chain_weight;
            O.net.big_cells = hv.big_cells;
            O.net.effort = hv.effort;
        }
        O.q_off = reinterpret_cast<const int64_t *>(d) + s0;
        O.e_off = reinterpret_cast<const int64_t *>(d + off_bytes) + s0;
        O.q_vars = reinterpret_cast<const int32_t *>(d + 3 * off_bytes);
        O.e_vars = O.q_vars + nq;
        O.B = m;
        O.flags = flags;
        O.orders = h->d_orders + s0 * 128;
        O.order_len = h->d_order_len + s0;
        O.scratch = h->d_order_scratch;
        O.zero = s0 == 0 ? h->d_emit_cursor : nullptr;
        O.perm = sorted ? reinterpret_cast<const int32_t *>(d + perm_off) + s0 : nullptr;
        O.lanes = plan_lanes_now(h);
        const int64_t per_wg = (int64_t)O.lanes * h->plan_waves;
        hipLaunchKernelGGL(order_kernel, dim3((unsigned)((m + per_wg - 1) / per_wg)), dim3(64 * h->plan_waves), 0, P, O);
        EmitArgs A;
        {   // the pointers of the device copy, the options of the moment
            A.net = h->net.emit_view();
            const EmitNet &dv = h->emit_net_dev;
            A.net.card = dv.card; A.net.log2card = dv.log2card; A.net.pool_off = dv.pool_off; A.net.scope_off = dv.scope_off;
            A.net.scope_vars = dv.scope_vars; A.net.scope_stride = dv.scope_stride; A.net.anc = dv.anc;
        }
        A.q_off = O.q_off;
        A.e_off = O.e_off;
        A.out_off = reinterpret_cast<const int64_t *>(d + 2 * off_bytes) + s0;
        A.q_vars = O.q_vars;
        A.e_vars = O.e_vars;
        A.e_codes = A.e_vars + ne;
        A.skip = reinterpret_cast<const char *>(A.e_codes + ne) + s0;
        A.orders = O.orders;
        A.order_len = O.order_len;
        A.B = m;
        A.flags = flags;
        A.prog = st.d_prog + (size_t)s0 * stride;
        A.prog_stride = (uint32_t)stride;
        A.meta = meta_out + s0;
        A.tags = tags_out;
        A.tag_cursor = h->d_emit_cursor;
        A.tag_cap = (uint32_t)tag_cap;
        A.scratch = h->d_emit_scratch;
        A.scratch_stride = scratch_stride;
        A.perm = O.perm;
        A.lanes = plan_lanes_now(h);
        hipLaunchKernelGGL(emit_kernel, dim3((unsigned)((m + per_wg - 1) / per_wg)), dim3(64 * h->plan_waves), 0, P, A);
        HIP_TRY(h, hipGetLastError());
    }
    HIP_TRY(h, hipEventRecord(h->emit_ev[1], P));
    return MIBN_OK;
}

// Waits for the device planner and fills `ck` for the n requests it planned, like plan_batch would (one "worker": the device).
// *dev_ms = duration of the kernels.  Returns MIBN_OK, an error, or 1 (see above).
int plan_on_device_collect(mibn_ctx *h, int64_t b0, int64_t n, BatchPlan &ck, double *dev_ms, std::vector<int64_t> *beyond_list) {
    hipStream_t P = h->search_stream;
    const size_t stride = h->emit_words;
    const size_t tag_cap = (size_t)n * 64;
    const EmitMeta *meta = reinterpret_cast<const EmitMeta *>(h->emit_out.get());
    const Tag *tags = reinterpret_cast<const Tag *>(h->emit_out.get() + (size_t)n * sizeof(EmitMeta) + 64);
    HIP_TRY(h, hipStreamSynchronize(P));
    {
        float ms = 0;
        HIP_TRY(h, hipEventElapsedTime(&ms, h->emit_ev[0], h->emit_ev[1]));
        if (dev_ms) *dev_ms = ms;
    }
    size_t n_tags = 0;  // (a request's items are contiguous, the requests' ranges in the order the lanes finished)
    for (int64_t i = 0; i < n; ++i)
        if (!meta[i].err) n_tags = std::max<size_t>(n_tags, (size_t)meta[i].tag_first + meta[i].n_tags);
    n_tags = std::min(n_tags, tag_cap);
    // the BatchPlan plan_batch would have filled (one "worker": the device)
    ck.st = PlanStats{};
    ck.arena_cells = 0;
    ck.err.clear();
    ck.prog_off.assign(n, 0);
    ck.cost.assign(n, 0.0);
    ck.arena_need.assign(n, 0);
    ck.thread_of.assign(n, 0);
    ck.local_off.assign(n, 0);
    ck.thread_words.clear();  // (nothing to upload: the programs are on the device)
    ck.tag_first.assign(n, 0);
    ck.tag_count.assign(n, 0);
    ck.tags.resize(1);
    ck.tags[0].assign(tags, tags + n_tags);
    bool refused = false, beyond = false;
    for (int64_t i = 0; i < n; ++i) {
        const EmitMeta &m = meta[i];
        if (m.err == kEmitErrWords) { refused = true; continue; }
        if (m.err == kEmitErrDevice) {  // beyond what wave_plan_kernel covers: the host plans this request (the chunk, if they are many)
            if (beyond_list && beyond_list->size() < 256) { beyond_list->push_back(i); continue; }
            refused = true; beyond = true; continue;
        }
        if (m.err) { h->err = "request " + std::to_string(b0 + i) + ": " + emit_error_message(m.err); return MIBN_E_LIMIT; }
        ck.prog_off[i] = (uint64_t)i * stride + m.prog_first;
        ck.local_off[i] = ck.prog_off[i];
        ck.tag_first[i] = m.tag_first;
        ck.tag_count[i] = m.n_tags;
        ck.cost[i] = m.alg_bytes;
        ck.arena_need[i] = m.arena_cells;
        ck.st.alg_bytes += m.alg_bytes;
        ck.st.alg_flops += m.alg_flops;
        ck.st.n_steps += m.n_steps;
        ck.st.max_step_cells = std::max(ck.st.max_step_cells, m.max_step_cells);
        ck.arena_cells = std::max(ck.arena_cells, m.arena_cells);
    }
    ck.total_words = (size_t)n * stride;
    if (refused) {
        if (h->trace || h->emit_fallbacks < 4) {  // (a rare event worth a line: the first few are always reported)
            int64_t nw = 0, nb = 0, first = -1;
            for (int64_t i = 0; i < n; ++i) { nw += meta[i].err == kEmitErrWords; nb += meta[i].err == kEmitErrDevice; if (meta[i].err && first < 0) first = i; }
            std::fprintf(stderr, "[mibn plan] device planner: %lld requests beyond a device limit, %lld did not fit their slot / the item buffer (first: request %lld, %u words, %u items; %zu items of %zu in the buffer): the host plans the chunk\n",
                         (long long)nb, (long long)nw, (long long)(b0 + first), first >= 0 ? meta[first].words : 0u, first >= 0 ? meta[first].n_tags : 0u, n_tags, tag_cap);
        }
        if (!beyond) h->emit_words = std::min<uint32_t>(h->emit_words * 2, 1u << 20);
        ++h->emit_fallbacks;
        return 1;
    }
    ++h->emit_chunks;
    return MIBN_OK;
}

// Small-network path (tiny_kernel.hip.h): the request arrays go to the device as they are, one lane answers one request,
// malformed requests are detected by the kernel (the host then re-validates to build the reference's message).
// Returns MIBN_OK / an error, or 1 when the batch does not fit the kernel and has to be planned.
constexpr int64_t kTinyZeroCopyRequests = 64;  // one wave

// mibn_expect_batch's device side: h->ex.plan over the results of the call in progress (device-resident, complete in stream order on the
// main stream) -> acc and p_out on the host.  expect_kernel per slab, expect_reduce_kernel over the cells the slabs touch, expect_big_kernel
// for the requests beyond the LDS image - in that order on the main stream: the addition order is the plan's.
int expect_run(mibn_t *h, const double *d_results) {
    mibn_ctx::Expect &X = h->ex;
    const ExpectPlan &P = X.plan;
    int rc;
    // one metadata buffer: the 8-byte arrays first
    std::vector<char> meta;
    auto put = [&](const void *src, size_t bytes) {
        const size_t o = meta.size();
        meta.resize(o + ((bytes + 7) & ~size_t(7)));
        if (bytes) std::memcpy(meta.data() + o, src, bytes);
        return o;
    };
    const size_t o_req = put(P.req.data(), P.req.size() * sizeof(ExpectReq)), o_big = put(P.big.data(), P.big.size() * sizeof(ExpectReq));
    const size_t o_ds = put(P.dim_stride.data(), P.dim_stride.size() * 8), o_sl = put(P.slab_lo.data(), P.slab_lo.size() * 8);
    const size_t o_sp = put(P.slab_part.data(), P.slab_part.size() * 8), o_dc = put(P.dim_card.data(), P.dim_card.size() * 4);
    const size_t o_sb = put(P.slab_begin.data(), P.slab_begin.size() * 4), o_sc = put(P.slab_cells.data(), P.slab_cells.size() * 4);
    const size_t o_bb = put(P.blk_begin.data(), P.blk_begin.size() * 4), o_bs = put(P.blk_slab.data(), P.blk_slab.size() * 4);
    if ((rc = ensure(h, X.d_meta, meta.size() + 16))) return rc;
    const size_t nB = (size_t)X.B, nA = (size_t)X.n_acc;
    const size_t f_acc = 0, f_p = nA, f_w = f_p + nB, f_part = f_w + (X.weight ? nB : 0);
    if ((rc = ensure(h, X.d_f64, f_part + (size_t)P.part_cells + 2))) return rc;
    for (Event &e : X.ev) HIP_TRY(h, e.ensure());
    const hipStream_t S = h->stream;
    HIP_TRY(h, hipMemcpyAsync(X.d_meta, meta.data(), meta.size(), hipMemcpyHostToDevice, S));
    if (nA) HIP_TRY(h, hipMemcpyAsync(X.d_f64 + f_acc, X.acc, nA * 8, hipMemcpyHostToDevice, S));
    if (X.weight) HIP_TRY(h, hipMemcpyAsync(X.d_f64 + f_w, X.weight, nB * 8, hipMemcpyHostToDevice, S));
    HIP_TRY(h, hipMemsetAsync(X.d_f64 + f_p, 0, nB * 8, S));
    const size_t n_slabs = P.slab_cells.size();
    double launches = 0;
    HIP_TRY(h, hipEventRecord(X.ev[0], S));
    if (n_slabs) {
        ExpectArgs A;
        A.results = d_results;
        A.req = reinterpret_cast<const ExpectReq *>(X.d_meta + o_req);
        A.dim_card = reinterpret_cast<const int32_t *>(X.d_meta + o_dc);
        A.dim_stride = reinterpret_cast<const int64_t *>(X.d_meta + o_ds);
        A.weight = X.weight ? X.d_f64 + f_w : nullptr;
        A.slab_begin = reinterpret_cast<const int32_t *>(X.d_meta + o_sb);
        A.slab_cells = reinterpret_cast<const int32_t *>(X.d_meta + o_sc);
        A.slab_part = reinterpret_cast<const int64_t *>(X.d_meta + o_sp);
        A.part = X.d_f64 + f_part;
        A.p_out = X.d_f64 + f_p;
        hipLaunchKernelGGL(expect_kernel, dim3((unsigned)n_slabs), dim3(64), 0, S, A);
        launches += 1;
    }
    if (P.n_blocks) {
        ExpectReduceArgs R;
        R.part = X.d_f64 + f_part;
        R.blk_begin = reinterpret_cast<const int32_t *>(X.d_meta + o_bb);
        R.blk_slab = reinterpret_cast<const int32_t *>(X.d_meta + o_bs);
        R.slab_lo = reinterpret_cast<const int64_t *>(X.d_meta + o_sl);
        R.slab_cells = reinterpret_cast<const int32_t *>(X.d_meta + o_sc);
        R.slab_part = reinterpret_cast<const int64_t *>(X.d_meta + o_sp);
        R.acc = X.d_f64 + f_acc;
        R.cell0 = P.cell0;
        R.n_acc = X.n_acc;
        hipLaunchKernelGGL(expect_reduce_kernel, dim3((unsigned)P.n_blocks), dim3(256), 0, S, R);
        launches += 1;
    }
    if (!P.big.empty()) {
        ExpectBigArgs G;
        G.results = d_results;
        G.req = reinterpret_cast<const ExpectReq *>(X.d_meta + o_big);
        G.dim_card = reinterpret_cast<const int32_t *>(X.d_meta + o_dc);
        G.dim_stride = reinterpret_cast<const int64_t *>(X.d_meta + o_ds);
        G.weight = X.weight ? X.d_f64 + f_w : nullptr;
        G.acc = X.d_f64 + f_acc;
        G.p_out = X.d_f64 + f_p;
        G.n_req = (int32_t)P.big.size();
        const unsigned grid = (unsigned)std::max<int64_t>(1, std::min<int64_t>(1024, (X.n_acc + kExpectBigWG - 1) / kExpectBigWG));
        hipLaunchKernelGGL(expect_big_kernel, dim3(grid), dim3(kExpectBigWG), 0, S, G);
        launches += 1;
    }
    HIP_TRY(h, hipEventRecord(X.ev[1], S));
    HIP_TRY(h, hipGetLastError());
    if (nA) HIP_TRY(h, hipMemcpyAsync(X.acc, X.d_f64 + f_acc, nA * 8, hipMemcpyDeviceToHost, S));
    if (X.p_out) HIP_TRY(h, hipMemcpyAsync(X.p_out, X.d_f64 + f_p, nB * 8, hipMemcpyDeviceToHost, S));
    HIP_TRY(h, hipStreamSynchronize(S));
    float ms = 0;
    HIP_TRY(h, hipEventElapsedTime(&ms, X.ev[0], X.ev[1]));
    book_stat(h, kStatExpect, launches, ms, 8.0 * ((double)(P.req.size() + P.big.size()) + 2.0 * (double)P.part_cells + 2.0 * (double)nA), (double)X.B, true, false);
    h->stats.kernel_ms += ms;
    h->stats.n_launches += launches;
    return MIBN_OK;
}

int run_tiny(mibn_t *h, uint32_t flags, int64_t B, const int64_t *q_off, const int32_t *q_vars, const int64_t *e_off,
             const int32_t *e_vars, const int32_t *e_codes, const int64_t *out_off, double *out, double t_start) {
    const size_t nq = (size_t)(q_off[B] - q_off[0]), ne = (size_t)(e_off[B] - e_off[0]);
    const size_t res_cells = (size_t)(out_off[B] - out_off[0]);
    if (q_off[0] != 0 || e_off[0] != 0) return 1;                    // (offsets relative to a larger array: plan)
    if (res_cells > (size_t)B * kTinyMaxQCells) return 1;
    int rc;
    // one pinned staging buffer: [q_off | e_off | out_off | q_vars | e_vars | e_codes | findings | bad | results (zero-copy calls only)]
    // findings (a call with likelihood findings: tiny_lh_kernel): [l_off | v_off | values | l_vars]
    const size_t off_bytes = (size_t)(B + 1) * 8;
    const size_t req_bytes = (3 * off_bytes + (nq + 2 * ne) * 4 + 15) & ~(size_t)15;
    const Findings *F = h->lh;
    const size_t nl = F ? F->l_vars.size() : 0, nv = F ? F->values.size() : 0;
    const size_t lh_bytes = F ? (off_bytes + (nl + 1) * 8 + nv * 8 + nl * 4 + 15) & ~(size_t)15 : 0;
    if (F && (nv >= (size_t)0x7fffffff || tiny_lds_bytes((int32_t)h->net.pool.size(), h->tiny_meta_words, true) > 65536)) return 1;  // (plan)
    // A call of at most one wave of requests (a single query(): BASELINE config 1) is latency, not bandwidth: the kernel reads the
    // request arrays from - and writes the posteriors and the bad-request flag to - the pinned, device-mapped staging buffer
    // itself.  No H2D / D2H copy, no timing events: one launch and one stream synchronisation (round 4 spent two DMAs each way
    // and two event records around a kernel of a few microseconds).  stats.kernel_ms is 0 for such a call.
    const bool zero_copy = B <= kTinyZeroCopyRequests && h->tiny_zero_copy && !h->expect;  // (expect_kernel reads the results on the device)
    const size_t bad_off = req_bytes + lh_bytes, res_off = bad_off + 16;
    const size_t bytes = res_off + (zero_copy ? res_cells * 8 : 0) + 64;
    PinnedBuf &sg = h->tiny_stage;
    if ((rc = pinned(h, sg, bytes))) return rc;
    if (!zero_copy) {
        if ((rc = ensure(h, h->d_tiny_req, bytes))) return rc;
        if ((rc = ensure(h, h->d_results[0], res_cells))) return rc;
    }
    char *p = sg.get();
    std::memcpy(p, q_off, off_bytes);
    std::memcpy(p + off_bytes, e_off, off_bytes);
    std::memcpy(p + 2 * off_bytes, out_off, off_bytes);
    char *pv = p + 3 * off_bytes;
    std::memcpy(pv, q_vars, nq * 4);
    if (ne) { std::memcpy(pv + nq * 4, e_vars, ne * 4); std::memcpy(pv + (nq + ne) * 4, e_codes, ne * 4); }
    const int32_t none = 0x7fffffff;
    if (F) {
        char *pl = p + req_bytes;
        std::memcpy(pl, F->l_off.data(), off_bytes);
        std::memcpy(pl + off_bytes, F->v_off.data(), (nl + 1) * 8);
        std::memcpy(pl + off_bytes + (nl + 1) * 8, F->values.data(), nv * 8);
        std::memcpy(pl + off_bytes + (nl + 1) * 8 + nv * 8, F->l_vars.data(), nl * 4);
    }
    std::memcpy(p + bad_off, &none, 4);
    char *dbase = h->d_tiny_req;  // where the kernel finds the arrays
    if (zero_copy) {
        void *dp = nullptr;
        HIP_TRY(h, hipHostGetDevicePointer(&dp, sg.get(), 0));
        dbase = static_cast<char *>(dp);
        std::memset(p + res_off, 0, res_cells * 8);
    } else {
        HIP_TRY(h, hipMemcpyAsync(h->d_tiny_req, p, bad_off + 16, hipMemcpyHostToDevice, h->stream));
    }
    TinyArgs A;
    A.pool = h->d_pool;
    A.meta = h->d_tiny_meta;
    A.q_off = reinterpret_cast<const int64_t *>(dbase);
    A.e_off = reinterpret_cast<const int64_t *>(dbase + off_bytes);
    A.out_off = reinterpret_cast<const int64_t *>(dbase + 2 * off_bytes);
    A.q_vars = reinterpret_cast<const int32_t *>(dbase + 3 * off_bytes);
    A.e_vars = A.q_vars + nq;
    A.e_codes = A.e_vars + ne;
    A.out = zero_copy ? reinterpret_cast<double *>(dbase + res_off) : h->d_results[0];
    A.bad = reinterpret_cast<int32_t *>(dbase + bad_off);
    A.B = B;
    A.n_vars = h->net.n_vars;
    A.pool_cells = (int32_t)h->net.pool.size();
    A.meta_words = h->tiny_meta_words;
    A.flags = (flags & ~kTinyFlagHostBad) | (zero_copy ? kTinyFlagHostBad : 0u);
    if (F) {
        const char *dl = dbase + req_bytes;
        A.l_off = reinterpret_cast<const int64_t *>(dl);
        A.v_off = reinterpret_cast<const int64_t *>(dl + off_bytes);
        A.values = reinterpret_cast<const double *>(dl + off_bytes + (nl + 1) * 8);
        A.l_vars = reinterpret_cast<const int32_t *>(dl + off_bytes + (nl + 1) * 8 + nv * 8);
    }
    const size_t lds = tiny_lds_bytes(A.pool_cells, A.meta_words, F != nullptr);
    const unsigned grid = (unsigned)std::max<int64_t>(1, std::min<int64_t>((B + 63) / 64, (int64_t)h->n_cu * 16));
    mibn_ctx::Set &st = h->set[0];
    if ((rc = retire(h, st))) return rc;
    size_t e0 = 0, e1 = 0;
    if (!zero_copy && (rc = next_event(h, st, e0))) return rc;
    hipLaunchKernelGGL(F ? tiny_lh_kernel : tiny_kernel, dim3(grid), dim3(64), lds, h->stream, A);
    HIP_TRY(h, hipGetLastError());
    if (!zero_copy && (rc = next_event(h, st, e1))) return rc;
    int32_t bad = none;
    const double t_d2h = now_ms();
    float ms = 0;
    if (zero_copy) {
        HIP_TRY(h, hipStreamSynchronize(h->stream));
        std::memcpy(&bad, p + bad_off, 4);
        std::memcpy(out + out_off[0], p + res_off, res_cells * 8);
    } else {
        HIP_TRY(h, hipMemcpyAsync(p + bad_off, h->d_tiny_req + bad_off, 4, hipMemcpyDeviceToHost, h->stream));
        if (!h->expect) HIP_TRY(h, hipMemcpyAsync(out + out_off[0], h->d_results[0], res_cells * 8, hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(h, hipStreamSynchronize(h->stream));
        std::memcpy(&bad, p + bad_off, 4);
        HIP_TRY(h, hipEventElapsedTime(&ms, st.ev[e0], st.ev[e1]));
    }
    h->stats.d2h_ms += now_ms() - t_d2h;
    st.ev_used = 0;
    if (bad != none) {  // the kernel skipped a malformed request: the message comes from the host-side checks
        Request rq;
        const int64_t b = bad;
        rq.nq = (int32_t)(q_off[b + 1] - q_off[b]);
        rq.qvars = q_vars + q_off[b];
        rq.ne = (int32_t)(e_off[b + 1] - e_off[b]);
        rq.evars = e_vars + e_off[b];
        rq.kind = (flags & MIBN_Q_UNNORMALISED) ? ProgramKind::Raw : ProgramKind::Sum;
        if (F) { rq.nl = (int32_t)(F->l_off[(size_t)b + 1] - F->l_off[(size_t)b]); rq.lvars = F->l_vars.data() + F->l_off[(size_t)b]; }
        std::string why = validate_request(h->net, rq);
        if (why.empty()) why = "out_off does not match the query table size";
        h->err = "request " + std::to_string(b) + ": " + why;
        return MIBN_E_ARG;
    }
    const double io_bytes = (double)bytes + 8.0 * (double)res_cells;
    h->stats.kernel_ms = ms;
    h->stats.n_launches = 1;
    h->stats.n_workgroups = grid;
    h->stats.alg_bytes = io_bytes;  // (request arrays in + posteriors out: nothing else touches HBM)
    h->stats.total_ms = now_ms() - t_start;
    h->total.kernel_ms += ms;
    h->total.n_launches += 1;
    h->total.alg_bytes += io_bytes;
    h->total.total_ms += h->stats.total_ms;
    h->total.d2h_ms += h->stats.d2h_ms;
    book_stat(h, F ? kStatTinyLh : kStatTiny, 1, ms, io_bytes, grid, true, true);
    if (h->expect) {
        if ((rc = expect_run(h, h->d_results[0]))) return rc;
        h->stats.total_ms = now_ms() - t_start;
    }
    return MIBN_OK;
}

// ---------------------------------------------------------------------------------------------- shared by the query driver and run_elim
// evidence labels outside their variables' domains: no program runs for the request (an empty posterior / zero probability)
bool evidence_outside_domain(const Network &net, const Request &rq, const int32_t *codes) {
    for (int i = 0; i < rq.ne; ++i)
        if (codes[i] < 0 || codes[i] >= net.card[rq.evars[i]]) return true;
    return false;
}

// The wave [r0, r1) of a chunk of n requests: consecutive requests whose private arenas fit the scratch budget together; a wave also
// ends once it holds `target` cells (kFullWaves: never - every wave as full as the budget allows).  `cells`: the wave's scratch.
constexpr int64_t kFullWaves = INT64_MAX;
int cut_wave(mibn_ctx *h, const std::vector<int64_t> &arena_need, int64_t r0, int64_t n, int64_t budget_cells, int64_t target, int64_t &r1, int64_t &cells) {
    for (r1 = r0, cells = 0; r1 < n; ++r1) {
        const int64_t need = (arena_need[(size_t)r1] + 15) & ~int64_t(15);
        if (r1 > r0 && (cells + need > budget_cells || cells >= target)) break;
        cells += need;
    }
    if (cells > budget_cells) { h->err = "a request needs " + std::to_string(8.0 * cells / 1e9) + " GB of scratch, above the arena budget"; return MIBN_E_NOMEM; }
    return MIBN_OK;
}

// The arena of `lane` holds need_bytes: grown with headroom (chunks differ by ~10 %: re-allocating tens of GB costs hundreds of ms),
// after S has drained - earlier launches of the lane still use the old arena.
int grow_arena(mibn_ctx *h, int lane, size_t need_bytes, int64_t budget_cells, hipStream_t S) {
    if (need_bytes <= h->d_arena[lane].cap()) return MIBN_OK;
    HIP_TRY(h, hipStreamSynchronize(S));
    HIP_TRY(h, h->d_arena[lane].reset(std::max(need_bytes, std::min((size_t)((double)budget_cells * 8.0), need_bytes + need_bytes / 3))));
    return MIBN_OK;
}

// The workers' program buffers of plan `ck`, back to back into d_prog from word `base` on.  Enqueued on `stream`, not waited for: `bufs`
// must stay as they are until the copies have run.
int upload_programs(mibn_ctx *h, uint32_t *d_prog, size_t base, const std::vector<ProgBuf> &bufs, const BatchPlan &ck, hipStream_t stream) {
    for (size_t t = 0; t < ck.thread_words.size(); ++t) {
        if (ck.thread_words[t]) HIP_TRY(h, hipMemcpyAsync(d_prog + base, bufs[t].data, ck.thread_words[t] * 4, hipMemcpyHostToDevice, stream));
        base += ck.thread_words[t];
    }
    return MIBN_OK;
}

// Likelihood findings (h->lh) of chunk [b0, b0 + n), planned into `ck`: the seed records of its requests and the chunk's packed weights
// -> cs, host and device.  Request r's seeds are the first cells of its arena in the order of its findings, each padded to 16 - what
// emit_begin gave them; a skipped request runs no program and gets no record.  Enqueued on `stream`, not waited for, out of cs.stage.
int upload_chunk_seeds(mibn_ctx *h, ChunkSeeds &cs, const BatchPlan &ck, int64_t b0, int64_t n, const char *skip, hipStream_t stream) {
    const Findings &F = *h->lh;
    int rc;
    cs.recs.clear();
    cs.first.assign((size_t)n + 1, 0);
    const int64_t v0 = F.v_off[(size_t)F.l_off[(size_t)b0]], v1 = F.v_off[(size_t)F.l_off[(size_t)(b0 + n)]];
    if (v1 - v0 >= (int64_t(1) << 32) || n >= (int64_t(1) << 31)) { h->err = "likelihood findings: too many weights in one chunk"; return MIBN_E_LIMIT; }
    for (int64_t r = 0; r < n; ++r) {
        const int64_t b = b0 + r;
        cs.first[(size_t)r] = (uint32_t)cs.recs.size();
        if (skip && skip[b]) continue;
        int64_t seed = 0;
        for (int64_t k = F.l_off[(size_t)b]; k < F.l_off[(size_t)b + 1]; ++k) {
            const int64_t cells = F.v_off[(size_t)k + 1] - F.v_off[(size_t)k];
            cs.recs.push_back({(uint32_t)r, (uint32_t)seed, (uint32_t)(F.v_off[(size_t)k] - v0), (uint32_t)cells});
            seed += (cells + 15) & ~int64_t(15);
        }
        if (seed > ck.arena_need[(size_t)r]) { h->err = "planner error: the seeds of request " + std::to_string(b) + " exceed its arena"; return MIBN_E_LIMIT; }
    }
    cs.first[(size_t)n] = (uint32_t)cs.recs.size();
    if (cs.recs.empty()) return MIBN_OK;
    if ((rc = ensure(h, cs.d_recs, cs.recs.size()))) return rc;
    if ((rc = ensure(h, cs.d_values, (size_t)(v1 - v0)))) return rc;
    const size_t rec_bytes = cs.recs.size() * sizeof(SeedRec), val_bytes = (size_t)(v1 - v0) * 8;
    if ((rc = pinned(h, cs.stage[0], rec_bytes))) return rc;
    if ((rc = pinned(h, cs.stage[1], val_bytes))) return rc;
    std::memcpy(cs.stage[0].get(), cs.recs.data(), rec_bytes);
    std::memcpy(cs.stage[1].get(), F.values.data() + v0, val_bytes);
    HIP_TRY(h, hipMemcpyAsync(cs.d_recs, cs.stage[0].get(), rec_bytes, hipMemcpyHostToDevice, stream));
    HIP_TRY(h, hipMemcpyAsync(cs.d_values, cs.stage[1].get(), val_bytes, hipMemcpyHostToDevice, stream));
    return MIBN_OK;
}

// The seed launch of wave [r0, r1) of that chunk: *SA and its grid, or false - the wave has no finding.
bool wave_seeds(const mibn_ctx *h, const ChunkSeeds &cs, int64_t r0, int64_t r1, double *arena, const uint64_t *d_arena_off, SeedArgs &SA, unsigned &grid, double &bytes) {
    if (!h->lh || cs.first.size() <= (size_t)r1 || cs.first[(size_t)r1] == cs.first[(size_t)r0]) return false;
    const uint32_t k0 = cs.first[(size_t)r0], k1 = cs.first[(size_t)r1];
    SA = SeedArgs{cs.d_recs + k0, cs.d_values, arena, d_arena_off, k1 - k0, (uint32_t)r0};
    grid = seed_grid(k1 - k0, h->n_cu);
    bytes = 0;
    for (uint32_t k = k0; k < k1; ++k) bytes += 16.0 * cs.recs[k].cells + sizeof(SeedRec);  // (weights in, seeds out, the record)
    return true;
}

// ---------------------------------------------------------------------------------------------- the query driver
// run_query: the driver behind mibn_query_batch, mibn_query_batch_ex, mibn_submit_batch and mibn_expect_batch - plan, upload and launch a
// batch.  Synchronous (ticket == nullptr): waits and writes `out`.  Asynchronous: the results land in a pinned buffer, *ticket identifies
// the call for mibn_wait; up to two calls may be in flight, so the host plans call s+1 while the GPU still runs call s.
// It is a sequence of stages over the call in flight (QueryRun); each says what it leaves enqueued, and not waited for, when it returns.
// Host memory that asynchronous work reads or writes is pinned and owned by the context - a set's st.bufs / st.xbufs and st.stage[],
// h->emit_in / h->emit_out, h->search_in / h->search_out, h->res_stage[] - never a local of a stage.  A stage returns MIBN_OK or the
// error it has set in h->err, wherever it stands: run_batch drains every stream before the caller sees an error (drained_on_error).
struct QueryRun {
    mibn_ctx *h;
    uint32_t flags;
    bool raw;  // MIBN_Q_UNNORMALISED
    int64_t B;
    const int64_t *q_off;
    const int32_t *q_vars;
    const int64_t *e_off;
    const int32_t *e_vars, *e_codes;
    const int64_t *out_off;
    double t_start;
    std::vector<char> skip;  // per request: 1 = evidence outside its domain (no steps), 2 = the empty product (the host writes it)
    int slot = 0;            // of h->d_results / h->pend
    double *d_results = nullptr;
    size_t res_cells = 0;
    int n_lanes = 1;
    int64_t budget_cells = 0;  // scratch budget of a lane
    bool lane1_used = false;
    bool emit_on = false, search_on = false;  // whole chunks planned on the device / the order search on the device, the emission on the host
    int64_t search_b0 = -1;                   // the search window: requests [search_b0, B) searched by one launch, waited for once (search_done)
    bool search_done = false, gpu_busy = false, short_first = false;
    int64_t n_chunks = 0;
    double call_fixed_ms = 0;  // the host's side of this call besides planning (the share rule of wave_plan_kernel)
    double call_plan_ms = 0;   // the workers' planning of the host's shares and the waits for the device planner: what the call's time to the last launch is NOT fixed cost
    bool host_only = false;    // MIBN_Q_UNNORMALISED or likelihood findings: planned by the host's workers - no device planner, no adaptive policy
};

// Stage: validation (bayes_net.py:840-845) and the out-of-domain-evidence short cut -> R.skip.  Nothing is enqueued.
int query_validate(QueryRun &R) {
    mibn_ctx *h = R.h;
    R.skip.assign((size_t)R.B, 0);
    for (int64_t b = 0; b < R.B; ++b) {
        Request rq;
        rq.nq = (int32_t)(R.q_off[b + 1] - R.q_off[b]);
        rq.qvars = R.q_vars + R.q_off[b];
        rq.ne = (int32_t)(R.e_off[b + 1] - R.e_off[b]);
        rq.evars = R.e_vars + R.e_off[b];
        rq.kind = R.raw ? ProgramKind::Raw : ProgramKind::Sum;
        if (h->lh) { rq.nl = (int32_t)(h->lh->l_off[(size_t)b + 1] - h->lh->l_off[(size_t)b]); rq.lvars = h->lh->l_vars.data() + h->lh->l_off[(size_t)b]; }
        if (!request_is_valid(h->net, rq)) { h->err = "request " + std::to_string(b) + ": " + validate_request(h->net, rq); return MIBN_E_ARG; }
        int64_t cells = 1;
        for (int i = 0; i < rq.nq; ++i) cells *= h->net.card[rq.qvars[i]];
        if (R.out_off[b + 1] - R.out_off[b] != cells) { h->err = "request " + std::to_string(b) + ": out_off does not match the query table size"; return MIBN_E_ARG; }
        if (evidence_outside_domain(h->net, rq, R.e_codes + R.e_off[b])) R.skip[(size_t)b] = 1;  // -> empty posterior
        // P(e) of empty evidence with pruning: the relevant set is empty and the program's FINAL step has no input - the empty
        // product, 1.0, which no kernel form computes: the host writes it after the download
        // (a finding makes its variable relevant: such a request has a program)
        if (R.raw && rq.nq == 0 && rq.ne == 0 && rq.nl == 0 && h->net.prune && !(R.flags & MIBN_Q_NOPRUNE)) R.skip[(size_t)b] = 2;
    }
    return MIBN_OK;
}

// Stage: call setup - the results buffer, the busy-time epoch, the arena budget and what this call plans where.  Enqueued on the main
// stream on return: the epoch record (an idle GPU), the zeroing of d_results and zero_ev, which lane 1's stream waits for.
int query_setup(QueryRun &R) {
    mibn_ctx *h = R.h;
    int rc;
    R.res_cells = (size_t)(R.out_off[R.B] - R.out_off[0]);
    if ((rc = ensure(h, h->d_results[R.slot], R.res_cells))) return rc;
    R.d_results = h->d_results[R.slot];
    R.n_lanes = h->n_streams > 1 ? 2 : 1;
    {
        bool idle = true;
        for (auto &st : h->set) idle = idle && !st.busy;
        if (!h->epoch) { HIP_TRY(h, h->epoch.ensure()); idle = true; }
        if (idle) {  // (times since the epoch stay small: float milliseconds)
            HIP_TRY(h, hipEventRecord(h->epoch, h->stream));
            h->busy_until = 0;
        }
    }
    HIP_TRY(h, hipMemsetAsync(R.d_results, 0, R.res_cells * 8, h->stream));
    if (R.n_lanes > 1) {  // lane 1 starts this call's work after the results buffer is zeroed
        HIP_TRY(h, h->zero_ev.ensure(hipEventDisableTiming));
        HIP_TRY(h, hipEventRecord(h->zero_ev, h->stream));
        HIP_TRY(h, hipStreamWaitEvent(h->stream2, h->zero_ev, 0));
    }
    size_t free_b = 0, total_b = 0;
    HIP_TRY(h, hipMemGetInfo(&free_b, &total_b));
    R.budget_cells = (int64_t)(std::min(h->arena_gb * 1e9, 0.8 * (double)(free_b + h->d_arena[0].cap() + h->d_arena[1].cap())) / 8.0) / R.n_lanes;
    // order_effort >= 1 (more candidate orders, the byte model's best two both emitted): the wave planner has it, order_kernel / emit_kernel do
    // not - where the wave planner does not cover the network the host plans (never two kinds of plans in one stream)
    bool effort_ok = true;
    if (h->net.order_effort >= 1 && (h->gpu_emit || h->gpu_search) && !R.host_only) {
        std::unique_ptr<WNet> probe(new WNet);
        effort_ok = h->wave_plan && h->net.wave_view(*probe);
    }
    R.emit_on = !R.host_only && h->gpu_emit && h->order_net_ok && h->emit_net_ok && effort_ok;
    // A rank that needs the device planner has no planning time to spare - and on the device the second emission costs more GPU time than
    // the bytes it saves give back (a two-thread rank: 243 against 273 k queries/s, profiles/r06_bh_ab.log): its calls take the extra
    // candidates only, on the host's share and on the device's alike.  (Like minfill_above below: the search effort follows the load.)
    h->net.second_above = (R.emit_on && !h->second_on_device) ? 1e300 : h->pol.base_second_above;
    R.search_on = !R.host_only && !R.emit_on && h->gpu_search && h->order_net_ok && h->net.order_effort < 1;
    // a short first chunk gets an idle GPU going while the host plans the first full-size one (first_chunk = 2: also when
    // an earlier asynchronous call still keeps the GPU busy; 0: never)
    for (auto &st : h->set) R.gpu_busy = R.gpu_busy || (st.busy && st.ev_used && hipEventQuery(st.ev[st.ev_used - 1]) == hipErrorNotReady);
    (void)hipGetLastError();  // (hipErrorNotReady is an answer, not an error: do not leave it for the check after the launches)
    R.short_first = h->first_chunk == 2 || (h->first_chunk == 1 && !R.gpu_busy);
    return MIBN_OK;
}

// Requests of the chunk that starts at b0.
// A call that finds the GPU idle (the first of a stream of calls, a blocking call) starts with a short chunk - a quarter -
// that gets the GPU going while the host plans the rest; in steady state - the previous call still running - a call
// is cut into full chunks.  (Ramping the chunks up from 1 024 requests, doubling, was measured and dropped: seven small
// plan_batch calls cost 95 ms of host time instead of 63, and the chunk sets - their pinned buffers sized by the small
// chunks they had seen - grew under the clock: profiles/r03_i_pipeline_start.log.)
// With the device order search on, every call starts with an eighth of a chunk whose orders the host searches while
// ONE launch searches the rest of the call (a call of a single chunk would otherwise be searched on the host whole).
int64_t chunk_size(const QueryRun &R, int64_t b0) {
    const mibn_ctx *h = R.h;
    if (b0 == 0 && R.search_on && h->gpu_search == 1) return std::max<int64_t>(1024, h->chunk / 8);
    if (R.emit_on) return h->chunk;  // (the host has nothing to plan while a short first chunk runs)
    if (b0 == 0 && R.short_first && (R.B > h->chunk || !R.gpu_busy)) return std::max<int64_t>(1024, h->chunk / 4);
    return h->chunk;
}

// plan_chunk, option gpu_search: the first (short) chunk of a call is searched on the host while one launch searches the rest of the
// call on the device; the later chunks only emit -> the orders of chunk [b0, b1), or null: the host searches.  Enqueued on return
// (first chunk only): order_kernel over [b1, B) on the search stream, from h->search_in into h->search_out.
int search_window(QueryRun &R, int64_t b0, int64_t b1, double t0, const uint8_t *&orders, const int32_t *&order_len) {
    mibn_ctx *h = R.h;
    int rc;
    if (h->gpu_search == 2) {  // test mode: every chunk searched on the device, synchronously
        if ((rc = search_orders_async(h, R.flags, b0, b1, R.q_off, R.q_vars, R.e_off, R.e_vars))) return rc;
        if ((rc = search_wait(h))) return rc;
        orders = reinterpret_cast<const uint8_t *>(h->search_out.get());
        order_len = reinterpret_cast<const int32_t *>(h->search_out.get() + (size_t)(b1 - b0) * 128);
    } else if (R.n_chunks == 0 && b1 < R.B) {
        if ((rc = search_orders_async(h, R.flags, b1, R.B, R.q_off, R.q_vars, R.e_off, R.e_vars))) return rc;
        R.search_b0 = b1;
    } else if (R.search_b0 >= 0) {
        if (!R.search_done) { if ((rc = search_wait(h))) return rc; R.search_done = true; h->search_ms += now_ms() - t0; }
        orders = reinterpret_cast<const uint8_t *>(h->search_out.get()) + (size_t)(b0 - R.search_b0) * 128;
        order_len = reinterpret_cast<const int32_t *>(h->search_out.get() + (size_t)(R.B - R.search_b0) * 128) + (b0 - R.search_b0);
    }
    return MIBN_OK;
}

// plan_chunk: joins the two parts of a chunk into `ck`, the device's nd requests (dp) first, the host's (hp: its programs follow the
// device's slots of `stride` words) behind them.  Returns prog_base.  Host work only.
size_t join_plans(BatchPlan &ck, BatchPlan &dp, BatchPlan &hp, int64_t nd, size_t stride) {
    const int T = (int)hp.tags.size();
    ck.st = dp.st;
    ck.st.alg_bytes += hp.st.alg_bytes; ck.st.alg_flops += hp.st.alg_flops; ck.st.n_steps += hp.st.n_steps;
    ck.st.max_step_cells = std::max(dp.st.max_step_cells, hp.st.max_step_cells);
    ck.arena_cells = std::max(dp.arena_cells, hp.arena_cells);
    ck.err.clear();
    ck.tags.resize((size_t)T + 1);
    for (int t = 0; t < T; ++t) ck.tags[(size_t)t].swap(hp.tags[(size_t)t]);
    ck.tags[(size_t)T].swap(dp.tags[0]);
    ck.thread_words = hp.thread_words;
    auto join = [&](auto &dst, const auto &a, const auto &b) { dst.assign(a.begin(), a.end()); dst.insert(dst.end(), b.begin(), b.end()); };
    join(ck.cost, dp.cost, hp.cost);
    join(ck.arena_need, dp.arena_need, hp.arena_need);
    join(ck.tag_first, dp.tag_first, hp.tag_first);
    join(ck.tag_count, dp.tag_count, hp.tag_count);
    join(ck.local_off, dp.local_off, hp.local_off);
    ck.thread_of.assign((size_t)nd, T);
    ck.thread_of.insert(ck.thread_of.end(), hp.thread_of.begin(), hp.thread_of.end());
    const size_t prog_base = (size_t)nd * stride;
    ck.prog_off = dp.prog_off;
    for (uint64_t o : hp.prog_off) ck.prog_off.push_back(prog_base + o);
    ck.total_words = prog_base + hp.total_words;
    return prog_base;
}

// plan_chunk: the requests `beyond` of the device's part [b0, b0 + nd) that exceed one of wave_plan_kernel's limits: the host plans THEM
// (round 6: a refused request used to send its whole chunk to the host - n_evidence = 16 met a limit five times in 200 000 requests and
// lost a third of its rate) - one plan_batch over the device's range with everything else masked out; a program goes into its
// request's own slot of the device program buffer, its work items and statistics take the place the kernel left empty.
// Enqueued on the copy stream on return: the copies of those programs from st.xbufs (pinned) into st.d_prog.
int replan_beyond(QueryRun &R, mibn_ctx::Set &st, int64_t b0, int64_t nd, const std::vector<int64_t> &beyond, bool &on_device) {
    mibn_ctx *h = R.h;
    BatchPlan &ck = st.plan, &xp = st.xplan;
    std::vector<char> mask(R.skip.begin(), R.skip.end());
    for (int64_t i = 0; i < nd; ++i) mask[(size_t)(b0 + i)] = 1;
    for (int64_t i : beyond) mask[(size_t)(b0 + i)] = R.skip[(size_t)(b0 + i)];
    plan_batch(h->net, *h->pool, st.xbufs, b0, b0 + nd, R.q_off, R.q_vars, R.e_off, R.e_vars, R.e_codes, R.out_off, mask.data(), xp,
               (R.flags & MIBN_Q_NOPRUNE) != 0, nullptr, nullptr, b0);
    if (!xp.err.empty()) { h->err = xp.err; return MIBN_E_LIMIT; }
    const size_t stride = h->emit_words;
    const size_t X = ck.tags.size();
    ck.tags.resize(X + xp.tags.size());
    for (size_t t = 0; t < xp.tags.size(); ++t) ck.tags[X + t] = xp.tags[t];
    bool fits = true;
    for (int64_t i : beyond) {
        const uint32_t *w = st.xbufs[(size_t)xp.thread_of[(size_t)i]].data + xp.local_off[(size_t)i];
        size_t words = 1;
        for (uint32_t k = 0; k < w[0]; ++k) words += w[words + 6];
        if (words + kMaxStepWords > stride) { fits = false; break; }
        HIP_TRY(h, hipMemcpyAsync(st.d_prog + (size_t)i * stride, w, words * 4, hipMemcpyHostToDevice, h->copy_stream));
        ck.prog_off[(size_t)i] = (uint64_t)i * stride;
        ck.local_off[(size_t)i] = ck.prog_off[(size_t)i];
        ck.thread_of[(size_t)i] = (int32_t)(X + (size_t)xp.thread_of[(size_t)i]);
        ck.tag_first[(size_t)i] = xp.tag_first[(size_t)i];
        ck.tag_count[(size_t)i] = xp.tag_count[(size_t)i];
        ck.cost[(size_t)i] = xp.cost[(size_t)i];
        ck.arena_need[(size_t)i] = xp.arena_need[(size_t)i];
    }
    ck.st.alg_bytes += xp.st.alg_bytes; ck.st.alg_flops += xp.st.alg_flops; ck.st.n_steps += xp.st.n_steps;
    ck.st.max_step_cells = std::max(ck.st.max_step_cells, xp.st.max_step_cells);
    ck.arena_cells = std::max(ck.arena_cells, xp.arena_cells);
    if (h->trace || h->emit_single < 4)
        std::fprintf(stderr, "[mibn plan] device planner: %zu of %lld requests beyond a device limit (first: request %lld): planned on the host\n", beyond.size(), (long long)nd,
                     (long long)(b0 + beyond[0]));
    h->emit_single += (int64_t)beyond.size();
    if (!fits) on_device = false;  // (a program longer than its slot: the host plans the chunk after all)
    return MIBN_OK;
}

// plan_chunk, option gpu_emit = 2 (tests): the host plans the device-planned chunk [b0, b1) too - programs, work items and statistics
// must agree exactly.  Synchronous: it waits for the copy stream and downloads st.d_prog; nothing is enqueued on return.
int check_against_host(QueryRun &R, mibn_ctx::Set &st, int64_t b0, int64_t b1) {
    mibn_ctx *h = R.h;
    const BatchPlan &ck = st.plan;
    const int64_t n = b1 - b0;
    const size_t stride = h->emit_words;
    std::vector<uint32_t> dev((size_t)n * stride);
    HIP_TRY(h, hipStreamSynchronize(h->copy_stream));  // (the programs of requests beyond a device limit, planned on the host: replan_beyond)
    HIP_TRY(h, hipMemcpy(dev.data(), st.d_prog, dev.size() * 4, hipMemcpyDeviceToHost));
    BatchPlan ref;
    plan_batch(h->net, *h->pool, st.bufs, b0, b1, R.q_off, R.q_vars, R.e_off, R.e_vars, R.e_codes, R.out_off, R.skip.data(), ref,
               (R.flags & MIBN_Q_NOPRUNE) != 0, nullptr, nullptr);
    if (!ref.err.empty()) { h->err = ref.err; return MIBN_E_LIMIT; }
    for (int64_t i = 0; i < n; ++i) {
        const uint32_t *hw = st.bufs[ref.thread_of[i]].data + ref.local_off[i], *dw = dev.data() + (size_t)ck.prog_off[(size_t)i];  // (= i x stride + the words in front of the program)
        size_t words = 1;
        for (uint32_t k = 0; k < hw[0]; ++k) words += hw[words + 6];
        for (size_t k = 0; k < words; ++k)
            if (hw[k] != dw[k]) {
                size_t off = 1, step = 0;  // (which step holds the word)
                while (step + 1 < hw[0] && off + hw[off + 6] <= k) { off += hw[off + 6]; ++step; }
                h->err = "device planner: request " + std::to_string(b0 + i) + " word " + std::to_string(k) + " of " + std::to_string(words) + " (step " + std::to_string(step) + " of " +
                         std::to_string(hw[0]) + ", kind " + std::to_string(hw[off] & 0xff) + ", word " + std::to_string(k - off) + " of the step's " + std::to_string(hw[off + 6]) + "): host " +
                         std::to_string(hw[k]) + " device " + std::to_string(dw[k]) + "; device program " + std::to_string(dw[0]) + " steps";
                return MIBN_E_STATE;
            }
        const Tag *ht = ref.tags[ref.thread_of[i]].data() + ref.tag_first[i], *dt = ck.tags[(size_t)ck.thread_of[i]].data() + ck.tag_first[i];
        bool same = ref.tag_count[i] == ck.tag_count[i] && ref.arena_need[i] == ck.arena_need[i] && ref.cost[i] == ck.cost[i];
        for (uint32_t k = 0; same && k < ref.tag_count[i]; ++k)
            same = ht[k].rel_off == dt[k].rel_off && ht[k].a == dt[k].a && ht[k].wgs == dt[k].wgs && ht[k].level == dt[k].level &&
                   ht[k].kid == dt[k].kid && ht[k].bytes == dt[k].bytes;
        if (!same) { h->err = "device planner: work items / statistics of request " + std::to_string(b0 + i) + " differ from the host's"; return MIBN_E_STATE; }
    }
    return MIBN_OK;
}

// Stage: plans chunk [b0, b1) into st.plan - on the host's workers (into st.bufs), on the device (into st.d_prog), or on both.
// on_device: st.d_prog already holds the device's programs, the host's (st.bufs) go behind them from word prog_base on.  The device
// planner has been waited for; enqueued on return: what search_window and replan_beyond leave.
int plan_chunk(QueryRun &R, mibn_ctx::Set &st, int64_t b0, int64_t b1, bool &on_device, size_t &prog_base) {
    mibn_ctx *h = R.h;
    const int64_t n = b1 - b0;
    const bool no_prune = (R.flags & MIBN_Q_NOPRUNE) != 0;
    int rc;
    const double t0 = now_ms();
    const uint8_t *orders = nullptr;
    const int32_t *order_len = nullptr;
    if (R.search_on && (rc = search_window(R, b0, b1, t0, orders, order_len))) return rc;
    BatchPlan &ck = st.plan;
    on_device = false;
    prog_base = 0;               // words of st.d_prog the device has written (the host's programs follow)
    std::vector<int64_t> beyond;  // requests of the device's part that exceed a device limit (kEmitErrDevice): the host plans them
    int64_t nd = 0;               // requests [b0, b0 + nd) planned by the device, the rest by the host's workers meanwhile
    if (R.emit_on) {
        nd = h->pol.device_share(n, h->gpu_emit == 2, wave_mode(h));
        const size_t stride = h->emit_words;
        if ((rc = plan_on_device_launch(h, R.flags, b0, b0 + nd, R.q_off, R.q_vars, R.e_off, R.e_vars, R.e_codes, R.out_off, R.skip.data(), st, (size_t)n * stride))) return rc;
        const double t_launched = now_ms();
        BatchPlan &hp = h->emit_host, &dp = h->emit_dev;
        double host_ms = 0, dev_ms = 0;
        if (nd < n) {
            const double th = now_ms();
            plan_batch(h->net, *h->pool, st.bufs, b0 + nd, b1, R.q_off, R.q_vars, R.e_off, R.e_vars, R.e_codes, R.out_off, R.skip.data(), hp, no_prune, nullptr, nullptr, b0);
            host_ms = now_ms() - th;
            R.call_plan_ms += host_ms;
            if (!hp.err.empty()) { h->err = hp.err; return MIBN_E_LIMIT; }
        }
        const double tw = now_ms();
        rc = plan_on_device_collect(h, b0, nd, nd < n ? dp : ck, &dev_ms, &beyond);
        h->emit_ms += now_ms() - tw;
        R.call_plan_ms += now_ms() - tw;
        if (h->trace >= 2) std::fprintf(stderr, "[mibn plan] collect returned %d at %.2f ms of the block\n", rc, now_ms() - t0);
        book_stat(h, kStatPlanner, 2, dev_ms, 0.0, (double)nd, true, true);  // (beside the chunk in flight: their time is not GPU busy time of its own)
#if defined(MIBN_EMIT_PROF)
        if (h->trace) {
            unsigned long long ticks[12], z[12] = {0};
            HIP_TRY(h, hipMemcpyFromSymbol(ticks, HIP_SYMBOL(g_emit_prof), sizeof(ticks)));
            HIP_TRY(h, hipMemcpyToSymbol(HIP_SYMBOL(g_emit_prof), z, sizeof(z)));
            static const char *names[11] = {"begin (relevant set, CPT slices)", "key / pos / slot sets", "factors of x", "sweep candidates", "SWEEP 5 / 4", "CHAIN",
                                            "SWEEP 3 / 2", "pair", "single elimination", "final product", "work items"};
            double tot = 0;
            for (int k = 0; k < 11; ++k) tot += (double)ticks[k];
            for (int k = 0; k < 11; ++k) std::fprintf(stderr, "[mibn emit phases] %-36s %6.1f us per request  %5.1f %%\n", names[k], (double)ticks[k] / 100.0 / (double)nd, 100.0 * (double)ticks[k] / tot);
        }
#endif
        if (h->trace) std::fprintf(stderr, "[mibn plan] chunk of %lld: device %lld requests (upload + launch %.2f ms, kernels %.2f ms, wait + collect %.2f ms), host %lld requests %.2f ms\n",
                                   (long long)n, (long long)nd, t_launched - t0, dev_ms, now_ms() - tw, (long long)(n - nd), host_ms);
        if (rc < 0 || rc > 1) return rc;
        if (rc == 0 && nd < n && hp.total_words > (size_t)(n - nd) * stride) rc = 1;  // (the host's programs do not fit behind the device's)
        on_device = rc == 0;
        if (on_device && nd < n) {
            prog_base = join_plans(ck, dp, hp, nd, stride);
            const bool wave = wave_mode(h);
            const PlanPolicy::ShareStep s = h->pol.after_mixed_chunk(n, nd, host_ms, dev_ms, h->chunk, wave);
            if (s.ruled && h->trace) std::fprintf(stderr, "[mibn share] host %.4f ms/request (%lld in %.1f ms), kernels %.5f ms/request, planner %.5f ms/request, fixed %.1f ms -> target %.3f, share %.3f\n",
                                                  s.ih, (long long)(n - nd), host_ms, s.kv, s.kp, s.fixed, s.target, h->pol.emit_share);
        }
    }
    if (on_device && !beyond.empty() && (rc = replan_beyond(R, st, b0, nd, beyond, on_device))) return rc;
    if (!on_device)
        plan_batch(h->net, *h->pool, st.bufs, b0, b1, R.q_off, R.q_vars, R.e_off, R.e_vars, R.e_codes, R.out_off, R.skip.data(), ck, no_prune, orders, order_len, -1, R.raw ? ProgramKind::Raw : ProgramKind::Sum,
                   h->lh ? h->lh->l_off.data() : nullptr, h->lh ? h->lh->l_vars.data() : nullptr);
    if (on_device && h->gpu_emit == 2 && (rc = check_against_host(R, st, b0, b1))) return rc;
    if (!ck.err.empty()) { h->err = ck.err; return MIBN_E_LIMIT; }
    for (auto &b : st.bufs)
        if (b.cap && !b.data) { h->err = "pinned host allocation failed"; return MIBN_E_HIP; }
    h->stats.plan_ms += now_ms() - t0;
    if (h->trace >= 2) std::fprintf(stderr, "[mibn plan] chunk planning block %.2f ms (on the device: %d)\n", now_ms() - t0, (int)on_device);
    return MIBN_OK;
}

// Stage: the programs the host planned and the program offsets of a chunk of n requests -> the set's device buffers.  Enqueued on the
// copy stream on return, not waited for: the copies out of st.bufs and st.stage[0] - and, for a call with likelihood findings, the
// chunk's seed records and weights out of st.seeds.stage - (run_wave's `uploaded` event covers them).
int upload_chunk(QueryRun &R, mibn_ctx::Set &st, int64_t b0, int64_t n, bool on_device, size_t prog_base) {
    mibn_ctx *h = R.h;
    const BatchPlan &ck = st.plan;
    int rc;
    if (!on_device && (rc = ensure(h, st.d_prog, ck.total_words + kMaxStepWords))) return rc;  // (slack: segment_wave prefetches whole descriptor slots)
    if ((rc = ensure(h, st.d_prog_off, (size_t)n))) return rc;
    if ((rc = ensure(h, st.d_arena_off, (size_t)n))) return rc;
    const double t0 = now_ms();
    if ((rc = upload_programs(h, st.d_prog, prog_base, st.bufs, ck, h->copy_stream))) return rc;
    if ((rc = upload(h, st.stage[0], st.d_prog_off, ck.prog_off.data(), (size_t)n * 8))) return rc;
    if (h->lh && (rc = upload_chunk_seeds(h, st.seeds, ck, b0, n, R.skip.data(), h->copy_stream))) return rc;
    h->stats.h2d_ms += now_ms() - t0;
    return MIBN_OK;
}

// The launches of a wave on the streams of its lane.  Option overlap: the sweep launch of a level goes to a second stream, next to the
// level kernel's launch of the same level (their items belong to different requests); level L + 1 starts on either stream when BOTH
// launches of level L have finished.  The tail of one launch - a sweep workgroup lives ~100 us - then runs under the body of the other.
// Streams of a wave: 0 = S, 1 .. 3 = the lane's aux streams; kLevelKernels says which kernel launches on which.  The launches of level L
// run side by side; a launch of level L + 1 waits for ALL launches of level L: the one on its own stream by stream order, the others
// through their end events (`prev`: the ends of the previous level - not the running `last`, or the launches of one level would
// serialise: ADVICE r3).  Without the option every launch goes to S and nothing waits.
//
// The kernels of a level, one row per LevelRoute (planner.h: route_of sends a class of work to its row, level_groups cuts a level's
// Launch entries into one launch per row).  A new kernel is one row here, one enumerator and one predicate in route_of, and - if it
// is to run beside the others - one more stream (kLevelStreams).  `slot`: the statistics slot of its launches; under split_kinds a
// launch is booked to its class id instead (LaunchGroup::stat_kid), except ve_sweep_dma_kernel's, which keep their slot.
struct LevelKernel { void (*kernel)(LevelArgs); unsigned block, lds_bytes; int stream, slot; };
constexpr LevelKernel kLevelKernels[kNumLevelRoutes] = {
    /* Level    */ {ve_level_kernel, kWG, 0, 0, kStatLevel},
    /* SweepDma */ {ve_sweep_dma_kernel, kSweepWG, kSweepLdsBytes, 1, kStatSweepDma},
    /* SweepReg */ {ve_sweep_kernel, kSweepWG, kSweepLdsBytes, 1, kKidSweep},
    /* Segment  */ {ve_segment_kernel, kWG, 0, 2, kStatSegment},
    /* Mfma     */ {ve_mfma_kernel, kWG, 0, 3, kStatMfma},
};
static_assert((int)LevelRoute::Level == 0 && (int)LevelRoute::SweepDma == 1 && (int)LevelRoute::SweepReg == 2 && (int)LevelRoute::Segment == 3 && (int)LevelRoute::Mfma == 4, "the rows' order");

struct LevelStreams {
    using Timed = mibn_ctx::Set::Timed;
    static constexpr int kNS = kLevelStreams;
    mibn_ctx *h;
    mibn_ctx::Set &st;
    const bool two;
    hipStream_t SS[kNS];
    long last[kNS], prev[kNS], saw[kNS][kNS];
    int cur_level = -1;
    Timed pair;  // the level in progress, as one concurrent launch group

    LevelStreams(mibn_ctx *h_, mibn_ctx::Set &st_, int lane, hipStream_t S)
        : h(h_), st(st_), two(h_->overlap != 0), SS{S, h_->aux[lane][0], h_->aux[lane][1], h_->aux[lane][2]}, pair(fresh()) {
        for (int a = 0; a < kNS; ++a) { last[a] = prev[a] = -1; for (int b = 0; b < kNS; ++b) saw[a][b] = -1; }
    }
    Timed fresh() const { return Timed{Timed::kLevelGroup, Timed::kNone, Timed::kNone, 0.0, 0.0, h->call_id}; }
    void close_pair() {
        if (std::any_of(std::begin(pair.e), std::end(pair.e), [](const size_t (&p)[2]) { return p[0] != Timed::kNone; })) st.timed.push_back(pair);
        pair = fresh();
    }
    // the wave's first event (the uploads, the previous wave's kernels: the arena is theirs until then) holds the other streams back
    int begin(size_t e_first) {
        for (int j = 1; two && j < kNS; ++j) HIP_TRY(h, hipStreamWaitEvent(SS[j], st.ev[e_first], 0));
        return MIBN_OK;
    }
    // in front of a launch of `level` on stream si: it waits for the previous level's launches on the other streams
    int before(int level, int si) {
        if (!two) return MIBN_OK;
        if (level != cur_level) { cur_level = level; for (int j = 0; j < kNS; ++j) prev[j] = last[j]; close_pair(); }
        for (int j = 0; j < kNS; ++j)
            if (j != si && prev[j] > saw[si][j]) { HIP_TRY(h, hipStreamWaitEvent(SS[si], st.ev[(size_t)prev[j]], 0)); saw[si][j] = prev[j]; }
        return MIBN_OK;
    }
    // behind it: events (e0, e1) bracket the launch
    void after(int si, size_t e0, size_t e1, double bytes, double grid) {
        if (!two) return;
        last[si] = (long)e1;
        if (h->split_kinds) return;
        pair.e[si][0] = e0; pair.e[si][1] = e1;
        pair.bytes += bytes;
        pair.items += grid;
    }
    // the wave ends on S
    int end() {
        if (!two) return MIBN_OK;
        close_pair();
        for (int j = 1; j < kNS; ++j)
            if (last[j] > saw[0][j]) HIP_TRY(h, hipStreamWaitEvent(SS[0], st.ev[(size_t)last[j]], 0));
        return MIBN_OK;
    }
};

// Stage: wave [r0, r1) of chunk [b0, ..) of set `st` on `lane` (stream S): the schedule, the arena, the uploads, the level launches.
// It waits for S when the arena has to grow, and for S and the copy stream when r0 > 0 (items / arena offsets of a wave live until the
// wave's launches have run: one wave per set at a time unless the chunk had to be split).  Enqueued on return, not waited for: on the
// copy stream the schedule's uploads out of st.stage[1..3] and the `uploaded` event; on S - and, option overlap, the lane's aux
// streams, joined back into S - the launches of every level between their events (st.ev, st.timed: retire() books them).
int run_wave(QueryRun &R, mibn_ctx::Set &st, int lane, hipStream_t S, int64_t b0, int64_t r0, int64_t r1) {
    mibn_ctx *h = R.h;
    int rc;
    double t0 = now_ms();
    Schedule &sc = st.sched;
    build_schedule(h->net, st.plan, st.bufs, r0, r1, sc);
    h->stats.plan_ms += now_ms() - t0;
    R.call_fixed_ms += now_ms() - t0;
    if (h->trace) std::fprintf(stderr, "[mibn plan] build_schedule %.2f ms (%zu items, %zu workgroups, %zu launches)\n", now_ms() - t0, sc.items.size(), sc.wg_item.size(), sc.launches.size());
    const size_t need_bytes = (size_t)std::max<int64_t>(16, sc.arena_cells) * sizeof(double);
    if ((rc = grow_arena(h, lane, need_bytes, R.budget_cells, S))) return rc;
    if (r0 > 0) { HIP_TRY(h, hipStreamSynchronize(S)); HIP_TRY(h, hipStreamSynchronize(h->copy_stream)); }
    if ((rc = ensure(h, st.d_items, sc.items.size()))) return rc;
    if ((rc = ensure(h, st.d_wg_item, sc.wg_item.size()))) return rc;
    t0 = now_ms();
    if ((rc = upload(h, st.stage[1], st.d_arena_off, sc.arena_off.data(), (size_t)(r1 - r0) * 8))) return rc;
    if ((rc = upload(h, st.stage[2], st.d_items, sc.items.data(), sc.items.size() * sizeof(Item)))) return rc;
    if ((rc = upload(h, st.stage[3], st.d_wg_item, sc.wg_item.data(), sc.wg_item.size() * sizeof(uint32_t)))) return rc;
    HIP_TRY(h, st.uploaded.ensure(hipEventDisableTiming));
    HIP_TRY(h, hipEventRecord(st.uploaded, h->copy_stream));
    HIP_TRY(h, hipStreamWaitEvent(S, st.uploaded, 0));  // the kernels of this wave wait for its uploads only
    h->stats.h2d_ms += now_ms() - t0;
    LevelArgs A;
    A.prog = st.d_prog;
    A.prog_off = st.d_prog_off + r0;
    A.arena_off = st.d_arena_off;
    A.pool = h->d_pool;
    A.arena = h->arena(lane);
    A.results = R.d_results + (R.out_off[b0] - R.out_off[0]);
    A.items = st.d_items;
    double n_wg = 0;
    if (h->trace) st.gap_from = h->n_waves ? (int)((h->n_waves - 1) & 3) : -1;
    // Every launch is bracketed by its own pair of events on its stream; the wave as a whole by the first and the last one on S
    // (retire() books the GPU's busy time from them).
    size_t e_first = 0, e_last = 0;
    if ((rc = next_event(h, st, e_first, S))) return rc;
    // likelihood findings: the seeds of the wave's requests, before any launch of its first level on any stream
    size_t e_begin = e_first;
    {
        SeedArgs SA;
        unsigned sgrid = 0;
        double sbytes = 0;
        if (wave_seeds(h, st.seeds, r0, r1, A.arena, st.d_arena_off, SA, sgrid, sbytes)) {
            size_t e0 = 0;
            if ((rc = next_event(h, st, e0, S))) return rc;
            hipLaunchKernelGGL(likelihood_seed_kernel, dim3(sgrid), dim3(kSeedWG), 0, S, SA);
            if ((rc = next_event(h, st, e_begin, S))) return rc;
            st.timed.push_back({kStatSeed, e0, e_begin, sbytes, (double)sgrid, h->call_id});
            n_wg += (double)sgrid;
        }
    }
    LevelStreams LS(h, st, lane, S);
    if ((rc = LS.begin(e_begin))) return rc;
    // one launch per group of a level's classes of work: planner.h level_groups, kLevelKernels
    level_groups(sc, {h->split_kinds != 0, h->seg_kernel != 0, h->mfma_kernel != 0, h->sweep_dma != 0}, st.groups);
    for (const LaunchGroup &g : st.groups) {
        const LevelKernel &K = kLevelKernels[(int)g.route];
        A.wg_item = st.d_wg_item + g.wg_level;
        A.wg_base = (uint32_t)(g.wg_first - g.wg_level);
        size_t e0 = 0, e1 = 0;
        const int si = LS.two ? K.stream : 0;
        hipStream_t Sx = LS.SS[si];
        if ((rc = LS.before(g.level, si))) return rc;
        if ((rc = next_event(h, st, e0, Sx))) return rc;
        hipLaunchKernelGGL(K.kernel, dim3((unsigned)g.grid), dim3(K.block), K.lds_bytes, Sx, A);
        if ((rc = next_event(h, st, e1, Sx))) return rc;
        LS.after(si, e0, e1, g.alg_bytes, (double)g.grid);
        st.timed.push_back({g.stat_kid >= 0 && g.route != LevelRoute::SweepDma ? g.stat_kid : K.slot, e0, e1, g.alg_bytes, (double)g.grid, h->call_id});
        n_wg += (double)g.grid;
    }
    if ((rc = LS.end())) return rc;
    if ((rc = next_event(h, st, e_last, S))) return rc;
    st.timed.push_back({mibn_ctx::Set::Timed::kWave, e_first, e_last, 0.0, (double)(r1 - r0), h->call_id});
    HIP_TRY(h, hipGetLastError());
    if (h->trace) {
        Event &ge = h->gap_ev[h->n_waves & 3];
        HIP_TRY(h, ge.ensure());
        HIP_TRY(h, hipEventRecord(ge, S));
    }
    ++h->n_waves;
    st.busy = true;
    h->stats.arena_bytes = std::max(h->stats.arena_bytes, (double)need_bytes);
    h->stats.n_workgroups += n_wg;
    return MIBN_OK;
}

// the host-side counters of the last call -> totals (kernel times are folded by retire())
void fold_stats(mibn_ctx *h) {
    h->total.plan_ms += h->stats.plan_ms;
    h->total.h2d_ms += h->stats.h2d_ms;
    h->total.d2h_ms += h->stats.d2h_ms;
    h->total.total_ms += h->stats.total_ms;
    h->total.alg_bytes += h->stats.alg_bytes;
    h->total.alg_flops += h->stats.alg_flops;
    h->total.n_steps += h->stats.n_steps;
    h->total.n_workgroups += h->stats.n_workgroups;
    h->total.arena_bytes = std::max(h->total.arena_bytes, h->stats.arena_bytes);
    h->total.max_step_cells = std::max(h->total.max_step_cells, h->stats.max_step_cells);
}

// Stage: completes the call.  Asynchronous (ticket): enqueued on the main stream on return, not waited for - the join of lane 1, the
// copy of the results into h->res_stage[slot] (pinned; mibn_wait copies it to `out`, which must stay valid until then) and the `done`
// event.  Synchronous: every set is retired, the results are downloaded to `out` (or handed to expect_run) and waited for.
int query_finish(QueryRun &R, double *out, int32_t *ticket) {
    mibn_ctx *h = R.h;
    int rc;
    if (R.lane1_used) {  // the download (main stream) follows the kernels of both lanes
        HIP_TRY(h, h->lane_ev.ensure(hipEventDisableTiming));
        HIP_TRY(h, hipEventRecord(h->lane_ev, h->stream2));
        HIP_TRY(h, hipStreamWaitEvent(h->stream, h->lane_ev, 0));
    }
    // (the fixed cost of a device-planned call is everything up to its last launch but the planning itself - validation, the fallbacks, the schedule,
    //  the uploads and some 600 launches: counting validation and schedule alone - 7.7 ms of 20 - left a two-thread rank host-bound once order_effort 1
    //  made its planning dearer, profiles/r06_bi_share.log)
    if (R.call_plan_ms > 0) R.call_fixed_ms = std::max(R.call_fixed_ms, now_ms() - R.t_start - R.call_plan_ms);
    if (!R.host_only) h->pol.call_end(R.B, R.call_fixed_ms);
    if (h->trace) std::fprintf(stderr, "[mibn plan] call of %lld requests: %.2f ms to the last launch (plan %.2f, h2d %.2f)\n", (long long)R.B, now_ms() - R.t_start, h->stats.plan_ms, h->stats.h2d_ms);
    if (ticket) {
        mibn_ctx::Pending &pd = h->pend[R.slot];
        PinnedBuf &sg = h->res_stage[R.slot];
        const size_t bytes = R.res_cells * 8;
        if ((rc = pinned(h, sg, bytes))) return rc;
        HIP_TRY(h, pd.done.ensure(hipEventDisableTiming));
        HIP_TRY(h, hipMemcpyAsync(sg.get(), R.d_results, bytes, hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(h, hipEventRecord(pd.done, h->stream));
        pd.active = true;
        pd.out = out + R.out_off[0];
        pd.cells = R.res_cells;
        h->next_slot ^= 1;
    } else {
        if ((rc = retire_all(h))) return rc;
        const double t0 = now_ms();
        if (h->expect) {  // mibn_expect_batch: the results stay on the device (a skipped request's slice is zero: it adds nothing)
            if ((rc = expect_run(h, R.d_results))) return rc;
        } else {
            HIP_TRY(h, hipMemcpyAsync(out + R.out_off[0], R.d_results, R.res_cells * 8, hipMemcpyDeviceToHost, h->stream));
            HIP_TRY(h, hipStreamSynchronize(h->stream));
        }
        h->stats.d2h_ms += now_ms() - t0;
        if (R.raw && !h->expect)
            for (int64_t b = 0; b < R.B; ++b)
                if (R.skip[(size_t)b] == 2) out[R.out_off[b]] = 1.0;  // (the empty product, see query_validate)
    }
    h->stats.total_ms = now_ms() - R.t_start;
    fold_stats(h);
    return MIBN_OK;
}

int run_query(mibn_t *h, uint32_t flags, int64_t B, const int64_t *q_off, const int32_t *q_vars, const int64_t *e_off, const int32_t *e_vars,
              const int32_t *e_codes, const int64_t *out_off, double *out, int32_t *ticket) {
    if (!h || B < 0 || !q_off || !e_off || !out_off || (B && !out && !h->expect)) return MIBN_E_ARG;
    if (int rc = check_state(h, kNeedDevice | kNeedNet)) return rc;
    QueryRun R{h, flags, (flags & MIBN_Q_UNNORMALISED) != 0, B, q_off, q_vars, e_off, e_vars, e_codes, out_off, now_ms()};
    R.host_only = R.raw || h->lh;
    ++h->call_id;
    h->search_ms = 0;
    h->emit_ms = 0;
    reset_last_stats(h);
    R.slot = h->next_slot;
    if (h->pend[R.slot].active) { h->err = "two asynchronous calls are already in flight: mibn_wait the older one first"; return MIBN_E_STATE; }
    if (ticket) *ticket = R.slot;
    if (B == 0) return MIBN_OK;
    HIP_TRY(h, hipSetDevice(h->device));
    if (h->tiny && h->tiny_ok && !ticket && B < 0x7ffffff0 && out_off[B] - out_off[0] >= B) {
        const int rc_tiny = run_tiny(h, flags | (h->net.prune ? 0u : (uint32_t)MIBN_Q_NOPRUNE), B, q_off, q_vars, e_off, e_vars, e_codes, out_off, out, R.t_start);
        if (rc_tiny != 1) return rc_tiny;  // 1: a request does not fit the kernel (query table too large) - plan it
    }
    // MIBN_Q_UNNORMALISED (P(q, e) / P(e) requests) and calls with likelihood findings: planned by the host's workers with the options'
    // base search effort - no device planner, no adaptive policy; the net's policy-tuned fields are restored on every exit
    struct NetEffort {
        Network *net = nullptr;
        double second_above = 0, minfill_above = 0;
        ~NetEffort() { if (net) { net->second_above = second_above; net->minfill_above = minfill_above; } }
    } keep_effort;
    if (R.host_only) {
        keep_effort.net = &h->net;
        keep_effort.second_above = h->net.second_above;
        keep_effort.minfill_above = h->net.minfill_above;
        h->net.minfill_above = h->pol.base_minfill;
    }
    int rc;
    if ((rc = query_validate(R))) return rc;
    ensure_pool(h);
    if (h->trace) std::fprintf(stderr, "[mibn plan] validation of %lld requests %.2f ms\n", (long long)B, now_ms() - R.t_start);
    R.call_fixed_ms = now_ms() - R.t_start;
    if (!R.host_only) {  // the adaptive policy (plan_policy.h) turns gpu_emit, gpu_search and the network's minfill_above
        const PlanPolicy::Knobs k = h->pol.call_start(h->call_id, (int)h->pool->size(), h->total.plan_ms, h->total.kernel_ms, h->retired_requests, h->order_net_ok,
                                                      h->emit_net_ok, {h->gpu_emit, h->gpu_search, h->net.minfill_above});
        h->gpu_emit = k.gpu_emit;
        h->gpu_search = k.gpu_search;
        h->net.minfill_above = k.minfill_above;
    }
    if ((rc = query_setup(R))) return rc;
    for (int64_t b0 = 0, b1 = 0; b0 < B; b0 = b1, ++R.n_chunks) {
        b1 = std::min(B, b0 + chunk_size(R, b0));
        const int64_t n = b1 - b0;
        mibn_ctx::Set &st = h->set[h->set_cursor];
        const int lane = R.n_lanes > 1 ? (h->set_cursor & 1) : 0;  // consecutive chunks alternate between the lanes
        hipStream_t S = lane ? h->stream2 : h->stream;
        R.lane1_used = R.lane1_used || lane == 1;
        h->set_cursor = (h->set_cursor + 1) % h->n_sets;
        if ((rc = retire(h, st))) return rc;  // its buffers are about to be rewritten
        bool on_device = false;
        size_t prog_base = 0;
        if ((rc = plan_chunk(R, st, b0, b1, on_device, prog_base))) return rc;
        if ((rc = upload_chunk(R, st, b0, n, on_device, prog_base))) return rc;
        // waves: consecutive requests whose private arenas fit the scratch budget together
        // (a chunk that does not fit is cut into waves of about EQUAL scratch - ceil(total / budget) of them - not into full
        //  waves and a remainder: round 4 runs chunks of 52 429 requests = 224 GB, close to the budget)
        const BatchPlan &ck = st.plan;
        int64_t chunk_cells = 0;
        for (int64_t r = 0; r < n; ++r) chunk_cells += (ck.arena_need[r] + 15) & ~int64_t(15);
        const int64_t n_waves_min = std::max<int64_t>(1, (chunk_cells + R.budget_cells - 1) / std::max<int64_t>(1, R.budget_cells));
        const int64_t wave_target = n_waves_min > 1 ? std::min(R.budget_cells, chunk_cells / n_waves_min + (chunk_cells / n_waves_min) / 64 + 1) : kFullWaves;
        for (int64_t r0 = 0, r1 = 0, cells = 0; r0 < n; r0 = r1) {
            if ((rc = cut_wave(h, ck.arena_need, r0, n, R.budget_cells, wave_target, r1, cells))) return rc;
            if ((rc = run_wave(R, st, lane, S, b0, r0, r1))) return rc;
        }
        h->stats.alg_bytes += ck.st.alg_bytes;
        h->stats.alg_flops += ck.st.alg_flops;
        h->stats.n_steps += ck.st.n_steps;
        h->stats.max_step_cells = std::max(h->stats.max_step_cells, ck.st.max_step_cells);
    }
    return query_finish(R, out, ticket);
}
}  // namespace

static int run_batch(mibn_t *h, uint32_t flags, int64_t B, const int64_t *q_off, const int32_t *q_vars, const int64_t *e_off, const int32_t *e_vars,
              const int32_t *e_codes, const int64_t *out_off, double *out, int32_t *ticket) {
    return drained_on_error(h, run_query(h, flags, B, q_off, q_vars, e_off, e_vars, e_codes, out_off, out, ticket), drain_streams_unchecked);
}

// ---------------------------------------------------------------------------------------------- blocking elimination calls
// run_elim: the one driver of the blocking, host-planned elimination calls - mibn_mpe_batch, mibn_posterior_sample_batch, mibn_map_batch.  It plans
// a chunk of requests on the workers (plan_batch), uploads the programs, cuts the chunk into waves by the arena budget, runs every
// wave level by level on the main stream and hands it to the payload for post-processing.  No tiny kernel, no device planner, no
// plan templates, no adaptive policy; the options are read, never written.  The arena of lane 0 is shared with the query calls
// (after the streams have drained); the buffers are mibn_ctx::Elim's; the statistics are those of the last call only.
//
// A payload supplies the flavour of the programs (kKind - for ProgramKind::Map with m_off / m_vars, the MAP variables - and no_prune: plan_batch), the level kernel with its
// statistics slot (launch_level, kLevelSlot), the limits its network must keep (limits: checked after the statistics reset and the
// B == 0 return, before the requests are validated - as each entry point always did), and three hooks.  Everything is on the main
// stream S; the driver owns every buffer of ElimRun::M but d_log_p, d_codes and d_draw_items, which are the payload's.
//   prepare(R)       once per chunk [b0, b0 + n).  Enqueued before it: the chunk's programs and prog_off (not waited for).  It
//                    initialises d_m[0 .. n) - the cell of request i of the chunk, which the FINAL step of its program overwrites and
//                    a skipped request (R.skip) never writes - and sizes its own buffers.  It may leave work enqueued; host memory
//                    it uploads from must stay valid until it has synchronised S itself.
//   after_levels(R)  once per wave [r0, r1) of the chunk.  Enqueued before it, not waited for: the wave's schedule and every level
//                    launch, whose launch errors the driver has already collected; d_m[r0 .. r1) and the arena (request i at
//                    M.d_arena_off[i - r0]) are complete in stream order.  It launches through R.timed_launch so that the time is
//                    booked, checks its own launch errors, and may leave work enqueued or synchronise S itself: the driver
//                    synchronises S after it in any case, before the next wave re-uses the arena and the schedule buffers.
//   download(R)      once per chunk, after its last wave has been synchronised: enqueues the copies of the chunk's results to the
//                    caller's arrays.  The driver synchronises S after it, before the next chunk re-uses d_m.
// A hook returns MIBN_OK or the error it has set in h->err; on any error the entry point drains the main stream (drained_on_error).
namespace {

struct ElimRun {  // the call in flight, as the hooks of a payload see it
    mibn_ctx *h;
    mibn_ctx::Elim &M;
    hipStream_t S;
    const char *skip;        // per request of the call: 1 = evidence outside its domain, no program runs (zero probability)
    int64_t b0 = 0, n = 0;   // the chunk: requests [b0, b0 + n) of the call
    int64_t r0 = 0, r1 = 0;  // the wave: requests [r0, r1) of the chunk
    size_t n_ev = 0;
    struct Timed { int slot; size_t e0, e1; double bytes, items; };
    std::vector<Timed> timed;  // the launches of the wave in flight

    int event(size_t &idx) {
        if (n_ev == M.ev.size()) M.ev.emplace_back();
        idx = n_ev++;
        HIP_TRY(h, M.ev[idx].ensure());
        HIP_TRY(h, hipEventRecord(M.ev[idx], S));
        return MIBN_OK;
    }
    // launch() between two events on S; its time is booked to statistics slot `slot` when the wave has been synchronised
    template <class Launch>
    int timed_launch(int slot, double bytes, double items, Launch &&launch) {
        size_t e0 = 0, e1 = 0;
        int rc;
        if ((rc = event(e0))) return rc;
        launch();
        if ((rc = event(e1))) return rc;
        timed.push_back({slot, e0, e1, bytes, items});
        return MIBN_OK;
    }
    int book() {
        for (const Timed &t : timed) {
            float ms = 0;
            HIP_TRY(h, hipEventElapsedTime(&ms, M.ev[t.e0], M.ev[t.e1]));
            book_stat(h, t.slot, 1, ms, t.bytes, t.items, true, false);
            h->stats.kernel_ms += ms;
            h->stats.n_launches += 1;
        }
        timed.clear();
        n_ev = 0;
        return MIBN_OK;
    }
};

template <class Payload>
int run_elim(mibn_ctx *h, int64_t B, const int64_t *e_off, const int32_t *e_vars, const int32_t *e_codes, Payload &P) {
    const double t_start = now_ms();
    reset_last_stats(h);
    if (B == 0) return MIBN_OK;
    const Network &net = h->net;
    int rc;
    if ((rc = P.limits(h))) return rc;
    // validation (unknown ids, duplicates) and the out-of-domain-evidence short cut
    std::vector<char> skip((size_t)B, 0);
    for (int64_t b = 0; b < B; ++b) {
        Request rq;
        rq.ne = (int32_t)(e_off[b + 1] - e_off[b]);
        rq.evars = e_vars + e_off[b];
        std::string e;
        if (h->lh) { rq.nl = (int32_t)(h->lh->l_off[(size_t)b + 1] - h->lh->l_off[(size_t)b]); rq.lvars = h->lh->l_vars.data() + h->lh->l_off[(size_t)b]; }
        if constexpr (Payload::kKind == ProgramKind::Map) {  // (the MAP variables too: unknown ids, duplicates, a variable both in M and in E)
            rq.nq = (int32_t)(P.m_off[b + 1] - P.m_off[b]);
            rq.qvars = P.m_vars + P.m_off[b];
            rq.kind = ProgramKind::Map;
            e = rq.ne < 0 || rq.nq < 0 ? std::string("negative count") : validate_request(net, rq);
        } else {
            e = rq.ne < 0 ? std::string("negative evidence count") : validate_mpe_request(net, rq);
        }
        if (!e.empty()) { h->err = "request " + std::to_string(b) + ": " + e; return MIBN_E_ARG; }
        if (evidence_outside_domain(net, rq, e_codes + e_off[b])) skip[(size_t)b] = 1;  // -> zero probability
    }
    HIP_TRY(h, hipSetDevice(h->device));
    ensure_pool(h);
    // an asynchronous query call may still use the arena of lane 0
    if ((rc = drain_streams(h))) return rc;
    ElimRun R{h, h->elim, h->stream, skip.data()};
    mibn_ctx::Elim &M = R.M;
    if (M.bufs.size() < (size_t)h->pool->size()) M.bufs.resize((size_t)h->pool->size());
    const hipStream_t S = R.S;
    std::vector<int64_t> q_off((size_t)B + 1, 0), out_off((size_t)B + 1);
    std::iota(out_off.begin(), out_off.end(), int64_t(0));  // one cell per request: d_m
    const int64_t *qo = q_off.data();  // (no query variables but a map program's M)
    const int32_t *qv = nullptr;
    if constexpr (Payload::kKind == ProgramKind::Map) { qo = P.m_off; qv = P.m_vars; }
    size_t free_b = 0, total_b = 0;
    HIP_TRY(h, hipMemGetInfo(&free_b, &total_b));
    const int64_t budget_cells = (int64_t)(std::min(h->arena_gb * 1e9, 0.8 * (double)(free_b + h->d_arena[0].cap())) / 8.0);
    for (int64_t b0 = 0, b1 = 0; b0 < B; b0 = b1) {
        b1 = std::min(B, b0 + std::max<int64_t>(1, h->chunk));
        const int64_t n = b1 - b0;
        R.b0 = b0;
        R.n = n;
        double t0 = now_ms();
        BatchPlan &ck = M.plan;
        plan_batch(net, *h->pool, M.bufs, b0, b1, qo, qv, e_off, e_vars, e_codes, out_off.data(), skip.data(), ck, P.no_prune,
                   nullptr, nullptr, -1, Payload::kKind, h->lh ? h->lh->l_off.data() : nullptr, h->lh ? h->lh->l_vars.data() : nullptr);
        if (!ck.err.empty()) { h->err = ck.err; return MIBN_E_LIMIT; }
        h->stats.plan_ms += now_ms() - t0;
        t0 = now_ms();
        if ((rc = ensure(h, M.d_prog, ck.total_words + kMaxStepWords))) return rc;  // (slack: segment_wave prefetches whole descriptor slots)
        if ((rc = ensure(h, M.d_prog_off, (size_t)n))) return rc;
        if ((rc = ensure(h, M.d_m, (size_t)n))) return rc;
        if ((rc = upload_programs(h, M.d_prog, 0, M.bufs, ck, S))) return rc;
        HIP_TRY(h, hipMemcpyAsync(M.d_prog_off, ck.prog_off.data(), (size_t)n * 8, hipMemcpyHostToDevice, S));
        if (h->lh && (rc = upload_chunk_seeds(h, M.seeds, ck, b0, n, skip.data(), S))) return rc;
        if ((rc = P.prepare(R))) return rc;
        h->stats.h2d_ms += now_ms() - t0;
        // waves: consecutive requests whose arenas (intermediates + what the payload's programs keep) fit the budget together
        for (int64_t r0 = 0, r1 = 0, cells = 0; r0 < n; r0 = r1) {
            if ((rc = cut_wave(h, ck.arena_need, r0, n, budget_cells, kFullWaves, r1, cells))) return rc;
            R.r0 = r0;
            R.r1 = r1;
            t0 = now_ms();
            Schedule &sc = M.sched;
            build_schedule(net, ck, M.bufs, r0, r1, sc);
            h->stats.plan_ms += now_ms() - t0;
            const size_t need_bytes = (size_t)std::max<int64_t>(16, sc.arena_cells) * sizeof(double);
            if ((rc = grow_arena(h, 0, need_bytes, budget_cells, S))) return rc;
            t0 = now_ms();
            if ((rc = ensure(h, M.d_arena_off, (size_t)(r1 - r0)))) return rc;
            if ((rc = ensure(h, M.d_items, std::max<size_t>(1, sc.items.size())))) return rc;
            if ((rc = ensure(h, M.d_wg_item, std::max<size_t>(1, sc.wg_item.size())))) return rc;
            HIP_TRY(h, hipMemcpyAsync(M.d_arena_off, sc.arena_off.data(), (size_t)(r1 - r0) * 8, hipMemcpyHostToDevice, S));
            if (!sc.items.empty()) HIP_TRY(h, hipMemcpyAsync(M.d_items, sc.items.data(), sc.items.size() * sizeof(Item), hipMemcpyHostToDevice, S));
            if (!sc.wg_item.empty()) HIP_TRY(h, hipMemcpyAsync(M.d_wg_item, sc.wg_item.data(), sc.wg_item.size() * sizeof(uint32_t), hipMemcpyHostToDevice, S));
            h->stats.h2d_ms += now_ms() - t0;
            LevelArgs A;
            A.prog = M.d_prog;
            A.prog_off = M.d_prog_off + r0;
            A.arena_off = M.d_arena_off;
            A.pool = h->d_pool;
            A.arena = h->arena(0);
            A.results = M.d_m;  // (FINAL offsets are chunk-relative: the cell of request b at b - b0)
            A.items = M.d_items;
            {   // likelihood findings: the seeds of the wave's requests, in stream order before its first level
                SeedArgs SA;
                unsigned sgrid = 0;
                double sbytes = 0;
                if (wave_seeds(h, M.seeds, r0, r1, A.arena, M.d_arena_off, SA, sgrid, sbytes)) {
                    if ((rc = R.timed_launch(kStatSeed, sbytes, (double)sgrid, [&] { hipLaunchKernelGGL(likelihood_seed_kernel, dim3(sgrid), dim3(kSeedWG), 0, S, SA); }))) return rc;
                    h->stats.n_workgroups += (double)sgrid;
                }
            }
            // one launch per level: every class of work of such a schedule (segments, GENERIC tiles) is the payload's level kernel's
            group_launches(sc, false, [](int) { return LevelRoute::Level; }, M.groups);
            for (const LaunchGroup &g : M.groups) {
                A.wg_item = M.d_wg_item + g.wg_level;
                A.wg_base = (uint32_t)(g.wg_first - g.wg_level);
                if ((rc = R.timed_launch(Payload::kLevelSlot, g.alg_bytes, (double)g.grid, [&] { P.launch_level((unsigned)g.grid, S, A); }))) return rc;
                h->stats.n_workgroups += (double)g.grid;
            }
            HIP_TRY(h, hipGetLastError());
            if ((rc = P.after_levels(R))) return rc;
            // the next wave re-uses the arena, the schedule buffers and the host schedule
            HIP_TRY(h, hipStreamSynchronize(S));
            h->stats.arena_bytes = std::max(h->stats.arena_bytes, (double)need_bytes);
            if ((rc = R.book())) return rc;
        }
        t0 = now_ms();
        if ((rc = P.download(R))) return rc;
        HIP_TRY(h, hipStreamSynchronize(S));
        h->stats.d2h_ms += now_ms() - t0;
        h->stats.alg_bytes += ck.st.alg_bytes;
        h->stats.alg_flops += ck.st.alg_flops;
        h->stats.n_steps += ck.st.n_steps;
        h->stats.max_step_cells = std::max(h->stats.max_step_cells, ck.st.max_step_cells);
    }
    h->stats.total_ms = now_ms() - t_start;
    return MIBN_OK;
}

// What the payloads share.  The masses a chunk starts from (DrawPayload, MapPayload): a skipped request never writes its cell - zero
// probability; a program without steps (nothing left after pruning, no evidence) has the empty product: 1, written here.  m_init is
// the caller's and is rewritten by the next chunk: the caller synchronises the stream before that.
int upload_initial_mass(ElimRun &R, std::vector<double> &m_init) {
    const mibn_ctx::Elim &M = R.M;
    const BatchPlan &ck = M.plan;
    m_init.assign((size_t)R.n, 0.0);
    for (int64_t i = 0; i < R.n; ++i)
        if (!R.skip[(size_t)(R.b0 + i)] && M.bufs[(size_t)ck.thread_of[(size_t)i]].data[ck.local_off[(size_t)i]] == 0) m_init[(size_t)i] = 1.0;
    HIP_TRY(R.h, hipMemcpyAsync(M.d_m, m_init.data(), (size_t)R.n * 8, hipMemcpyHostToDevice, R.S));
    return MIBN_OK;
}

// The traceback of the wave's requests (MpePayload, MapPayload): everything but where the codes go.
TracebackArgs traceback_args(const ElimRun &R) {
    TracebackArgs T;
    T.prog = R.M.d_prog;
    T.prog_off = R.M.d_prog_off + R.r0;
    T.arena_off = R.M.d_arena_off;
    T.arena = R.h->arena(0);
    T.m = R.M.d_m + R.r0;
    T.m_off = nullptr;
    T.codes = nullptr;
    T.log_p = R.M.d_log_p + R.r0;
    T.n_req = (uint32_t)(R.r1 - R.r0);
    T.n_vars = R.h->net.n_vars;
    return T;
}

// ---------------------------------------------------------------------------------------------- most probable explanation
// mibn_mpe_batch: max programs (planner.h) run by ve_max_kernel - the arena of a request holds its intermediates and argmax tables -,
// decoded wave by wave by mpe_traceback_kernel, downloaded chunk by chunk.
struct MpePayload {
    static constexpr ProgramKind kKind = ProgramKind::Max;
    static constexpr bool no_prune = false;
    static constexpr int kLevelSlot = kStatMax;
    int32_t *codes;
    double *log_p;

    int limits(mibn_ctx *h) const {
        for (int v = 0; v < h->net.n_vars; ++v)
            if (h->net.card[v] > 65536) { h->err = "mpe: variable " + std::to_string(v) + " has more than 65 536 states (argmax entries are 16 bits)"; return MIBN_E_LIMIT; }
        return MIBN_OK;
    }
    void launch_level(unsigned grid, hipStream_t S, const LevelArgs &A) const { hipLaunchKernelGGL(ve_max_kernel, dim3(grid), dim3(kWG), 0, S, A); }
    int prepare(ElimRun &R) const {
        mibn_ctx *h = R.h;
        int rc;
        if ((rc = ensure(h, R.M.d_log_p, (size_t)R.n))) return rc;
        if ((rc = ensure(h, R.M.d_codes, (size_t)R.n * (size_t)std::max(1, h->net.n_vars)))) return rc;
        HIP_TRY(h, hipMemsetAsync(R.M.d_m, 0, (size_t)R.n * 8, R.S));  // (skipped requests never write theirs: zero probability)
        return MIBN_OK;
    }
    int after_levels(ElimRun &R) const {
        mibn_ctx *h = R.h;
        TracebackArgs T = traceback_args(R);
        T.codes = R.M.d_codes + (size_t)R.r0 * (size_t)h->net.n_vars;
        int rc;
        if ((rc = R.timed_launch(kStatTraceback, 0.0, (double)(R.r1 - R.r0), [&] {
                hipLaunchKernelGGL(mpe_traceback_kernel, dim3((unsigned)(R.r1 - R.r0)), dim3(kTracebackWG), 0, R.S, T);
            })))
            return rc;
        HIP_TRY(h, hipGetLastError());
        return MIBN_OK;
    }
    int download(ElimRun &R) const {
        mibn_ctx *h = R.h;
        const size_t nv = (size_t)h->net.n_vars;
        HIP_TRY(h, hipMemcpyAsync(codes + (size_t)R.b0 * nv, R.M.d_codes, (size_t)R.n * nv * 4, hipMemcpyDeviceToHost, R.S));
        HIP_TRY(h, hipMemcpyAsync(log_p + R.b0, R.M.d_log_p, (size_t)R.n * 8, hipMemcpyDeviceToHost, R.S));
        return MIBN_OK;
    }
};

// ---------------------------------------------------------------------------------------------- exact posterior sampling
// mibn_posterior_sample_batch: draw programs (planner.h) run by ve_sum_kernel - once per request, whatever its number of samples; every
// table is kept in the arena -, then posterior_draw_kernel walks each request's draw record once per sample, in launches of at most
// kDrawCodeWords code words whose rows are downloaded before the next one.
constexpr size_t kDrawCodeWords = size_t(64) << 20;  // 256 MB of codes on the device per draw launch

struct DrawPayload {
    static constexpr ProgramKind kKind = ProgramKind::Draw;
    static constexpr int kLevelSlot = kStatSum;
    const bool no_prune;
    const int64_t *s_off;
    const uint64_t seed;
    int32_t *codes;
    double *p_e;
    bool wide = false;  // limits: a variable of more than 256 states (16-bit sample states)
    size_t lds = 0;     // limits: the LDS-resident sample state of a workgroup
    std::vector<double> m_init, gather;
    std::vector<DrawItem> ditems;

    int limits(mibn_ctx *h) {
        const int nv = h->net.n_vars;
        for (int v = 0; v < nv; ++v) {
            if (h->net.card[v] > 65536) { h->err = "posterior sampling: variable " + std::to_string(v) + " has more than 65 536 states (sample states are 16 bits)"; return MIBN_E_LIMIT; }
            wide = wide || h->net.card[v] > 256;
        }
        lds = draw_lds_bytes(nv, wide);
        if (lds > 150 * 1024) { h->err = "posterior sampling: network too large for the LDS-resident sample state"; return MIBN_E_LIMIT; }
        return MIBN_OK;
    }
    void launch_level(unsigned grid, hipStream_t S, const LevelArgs &A) const { hipLaunchKernelGGL(ve_sum_kernel, dim3(grid), dim3(kWG), 0, S, A); }
    int prepare(ElimRun &R) {
        mibn_ctx *h = R.h;
        const mibn_ctx::Elim &M = R.M;
        const BatchPlan &ck = M.plan;
        const int64_t n = R.n;
        int rc;
        if (R.b0 == 0 && lds > 64 * 1024) {  // (once per call, before the first draw launch)
            HIP_TRY(h, hipFuncSetAttribute((const void *)posterior_draw_kernel<uint8_t>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
            HIP_TRY(h, hipFuncSetAttribute((const void *)posterior_draw_kernel<uint16_t>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        }
        if ((rc = upload_initial_mass(R, m_init))) return rc;
        HIP_TRY(h, hipStreamSynchronize(R.S));  // (m_init is rewritten by the next chunk)
        // table bytes one sample of each request gathers (the draw kernel's "algorithmic bytes"): 8 per input and state of every entry
        gather.assign((size_t)n, 0.0);
        for (int64_t i = 0; i < n; ++i) {
            const uint32_t *p = M.bufs[(size_t)ck.thread_of[(size_t)i]].data + ck.local_off[(size_t)i];
            const uint32_t *rec = p + record_offset(p);
            const uint32_t n_ent = rec[0] + rec[1];
            rec += 3 + 2 * rec[2];
            for (uint32_t e = 0; e < n_ent; ++e) {
                const uint32_t cx = rec[1], n_in = rec[2];
                rec += 3;
                for (uint32_t j = 0; j < n_in; ++j) rec += 4 + 2 * rec[3];
                gather[(size_t)i] += 8.0 * (double)cx * (double)n_in;
            }
        }
        return MIBN_OK;
    }
    // the draws of the wave's requests: workgroups of up to kDrawWG consecutive samples of one request, launched in groups of at most
    // rows_cap rows (consecutive rows of `codes`: the requests of a wave are consecutive)
    int after_levels(ElimRun &R) {
        mibn_ctx *h = R.h;
        mibn_ctx::Elim &M = R.M;
        const hipStream_t S = R.S;
        const int nv = h->net.n_vars;
        const int64_t b0 = R.b0, r0 = R.r0, r1 = R.r1;
        const size_t rows_cap = std::max<size_t>(kDrawWG, kDrawCodeWords / (size_t)std::max(1, nv));
        DrawArgs D;
        D.prog = M.d_prog;
        D.prog_off = M.d_prog_off + r0;
        D.arena_off = M.d_arena_off;
        D.arena = h->arena(0);
        D.pool = h->d_pool;
        D.m = M.d_m + r0;
        D.n_vars = nv;
        D.k0 = (uint32_t)seed;
        D.k1 = (uint32_t)(seed >> 32) ^ 0x85EBCA6Bu;  // (the key of mibn_sample)
        int rc;
        int64_t rb = r0, sb = s_off[b0 + r0];  // next sample to place: request rb, global row sb
        while (rb < r1) {
            ditems.clear();
            const int64_t g_first = sb;
            size_t rows = 0;
            double gbytes = 0;
            while (rb < r1 && rows < rows_cap) {
                const int64_t end = s_off[b0 + rb + 1];
                if (sb >= end) { ++rb; if (rb < r1) sb = s_off[b0 + rb]; continue; }
                const int64_t cnt = std::min<int64_t>({(int64_t)kDrawWG, end - sb, (int64_t)(rows_cap - rows)});
                ditems.push_back(DrawItem{(uint32_t)(rb - r0), (uint32_t)cnt, (uint64_t)sb, (uint64_t)(sb - g_first)});
                sb += cnt;
                rows += (size_t)cnt;
                gbytes += (double)cnt * gather[(size_t)rb];
            }
            if (ditems.empty()) break;
            double t0 = now_ms();
            if ((rc = ensure(h, M.d_draw_items, ditems.size()))) return rc;
            if ((rc = ensure(h, M.d_codes, rows * (size_t)std::max(1, nv)))) return rc;
            HIP_TRY(h, hipMemcpyAsync(M.d_draw_items, ditems.data(), ditems.size() * sizeof(DrawItem), hipMemcpyHostToDevice, S));
            h->stats.h2d_ms += now_ms() - t0;
            D.items = M.d_draw_items;
            D.codes = M.d_codes;
            if ((rc = R.timed_launch(kStatDraw, gbytes, (double)rows, [&] {
                    if (wide) hipLaunchKernelGGL(posterior_draw_kernel<uint16_t>, dim3((unsigned)ditems.size()), dim3(kDrawWG), lds, S, D);
                    else hipLaunchKernelGGL(posterior_draw_kernel<uint8_t>, dim3((unsigned)ditems.size()), dim3(kDrawWG), lds, S, D);
                })))
                return rc;
            h->stats.n_workgroups += (double)ditems.size();
            HIP_TRY(h, hipGetLastError());
            t0 = now_ms();
            if (nv > 0)
                HIP_TRY(h, hipMemcpyAsync(codes + (size_t)(g_first - s_off[0]) * (size_t)nv, M.d_codes, rows * (size_t)nv * 4, hipMemcpyDeviceToHost, S));
            HIP_TRY(h, hipStreamSynchronize(S));  // (the next group re-uses the items and the codes)
            h->stats.d2h_ms += now_ms() - t0;
        }
        return MIBN_OK;
    }
    int download(ElimRun &R) const {
        if (p_e) HIP_TRY(R.h, hipMemcpyAsync(p_e + R.b0, R.M.d_m, (size_t)R.n * 8, hipMemcpyDeviceToHost, R.S));
        return MIBN_OK;
    }
};

// ---------------------------------------------------------------------------------------------- marginal MAP
// mibn_map_batch: map programs (planner.h) run by ve_map_kernel - sum steps and max steps in one schedule; the arena of a request holds
// its intermediates and the argmax tables of its max steps -, decoded wave by wave by map_traceback_kernel into the requests' slices of
// d_codes, downloaded chunk by chunk.
struct MapPayload {
    static constexpr ProgramKind kKind = ProgramKind::Map;
    static constexpr int kLevelSlot = kStatMap;
    const bool no_prune;
    const int64_t B;
    const int64_t *m_off;
    const int32_t *m_vars;
    int32_t *codes;
    double *log_p;
    std::vector<double> m_init;
    std::vector<int64_t> rel_off;  // m_off of the chunk, relative to its first request

    int limits(mibn_ctx *h) const {
        for (int64_t k = m_off[0]; k < m_off[B]; ++k) {
            const int32_t v = m_vars[k];
            if (v >= 0 && v < h->net.n_vars && h->net.card[v] > 65536) {
                h->err = "map: variable " + std::to_string(v) + " has more than 65 536 states (argmax entries are 16 bits)";
                return MIBN_E_LIMIT;
            }
        }
        return MIBN_OK;
    }
    void launch_level(unsigned grid, hipStream_t S, const LevelArgs &A) const { hipLaunchKernelGGL(ve_map_kernel, dim3(grid), dim3(kWG), 0, S, A); }
    int prepare(ElimRun &R) {
        mibn_ctx *h = R.h;
        const mibn_ctx::Elim &M = R.M;
        const int64_t n = R.n;
        int rc;
        if ((rc = ensure(h, R.M.d_log_p, (size_t)n))) return rc;
        if ((rc = ensure(h, R.M.d_m_off, (size_t)n + 1))) return rc;
        if ((rc = ensure(h, R.M.d_codes, (size_t)std::max<int64_t>(1, m_off[R.b0 + n] - m_off[R.b0])))) return rc;
        rel_off.resize((size_t)n + 1);
        for (int64_t i = 0; i <= n; ++i) rel_off[(size_t)i] = m_off[R.b0 + i] - m_off[R.b0];
        if ((rc = upload_initial_mass(R, m_init))) return rc;
        HIP_TRY(h, hipMemcpyAsync(M.d_m_off, rel_off.data(), ((size_t)n + 1) * 8, hipMemcpyHostToDevice, R.S));
        HIP_TRY(h, hipStreamSynchronize(R.S));  // (both vectors are rewritten by the next chunk)
        return MIBN_OK;
    }
    int after_levels(ElimRun &R) const {
        mibn_ctx *h = R.h;
        const mibn_ctx::Elim &M = R.M;
        // what the wave's level launches held beside segments: the tiled steps of either kind (statistics only)
        for (const Item &it : M.sched.items) {
            if (it.a & kItemSegment) continue;
            const size_t r = (size_t)R.r0 + it.req;
            const uint32_t *w = M.bufs[(size_t)M.plan.thread_of[r]].data + M.plan.local_off[r] + it.rel_off;
            const int th = std::max(1, (int)it.a);
            book_stat(h, ((w[1] >> 16) & kFlagMax) ? kStatMapMaxTiles : kStatMapSumTiles, 1, 0.0, 0.0,  // (their bytes are ve_map_kernel's)
                      (double)(((int64_t)w[3] + th - 1) / th), true, false);
        }
        TracebackArgs T = traceback_args(R);
        T.m_off = M.d_m_off + R.r0;
        T.codes = M.d_codes;
        int rc;
        if ((rc = R.timed_launch(kStatMapTraceback, 0.0, (double)(R.r1 - R.r0), [&] {
                hipLaunchKernelGGL(map_traceback_kernel, dim3((unsigned)(R.r1 - R.r0)), dim3(kTracebackWG), 0, R.S, T);
            })))
            return rc;
        HIP_TRY(h, hipGetLastError());
        return MIBN_OK;
    }
    int download(ElimRun &R) const {
        mibn_ctx *h = R.h;
        const int64_t cells = m_off[R.b0 + R.n] - m_off[R.b0];
        if (cells > 0) HIP_TRY(h, hipMemcpyAsync(codes + (m_off[R.b0] - m_off[0]), R.M.d_codes, (size_t)cells * 4, hipMemcpyDeviceToHost, R.S));
        HIP_TRY(h, hipMemcpyAsync(log_p + R.b0, R.M.d_log_p, (size_t)R.n * 8, hipMemcpyDeviceToHost, R.S));
        return MIBN_OK;
    }
};

// The argument checks of each entry point come first, in its own order; then the driver.
int run_mpe_body(mibn_t *h, int64_t B, const int64_t *e_off, const int32_t *e_vars, const int32_t *e_codes, int32_t *codes, double *log_p) {
    if (!h || B < 0 || !e_off || (B && (!codes || !log_p))) return MIBN_E_ARG;
    if (int rc = check_state(h, kNeedDevice | kNeedNet)) return rc;
    MpePayload P{codes, log_p};
    return run_elim(h, B, e_off, e_vars, e_codes, P);
}

int run_draw_body(mibn_t *h, int64_t B, const int64_t *e_off, const int32_t *e_vars, const int32_t *e_codes, const int64_t *s_off,
                  uint64_t seed, uint32_t flags, int32_t *codes, double *p_e) {
    if (!h || B < 0 || !e_off || !s_off) return MIBN_E_ARG;
    if (int rc = check_state(h, kNeedDevice | kNeedNet)) return rc;
    if (flags & ~(uint32_t)MIBN_DRAW_PRUNE) { h->err = "posterior sampling: unknown flag"; return MIBN_E_ARG; }
    for (int64_t b = 0; b < B; ++b)
        if (s_off[b + 1] < s_off[b] || s_off[b] < 0) { h->err = "posterior sampling: s_off must be non-negative and ascending"; return MIBN_E_ARG; }
    if (B && s_off[B] > s_off[0] && !codes) return MIBN_E_ARG;
    DrawPayload P{!(flags & MIBN_DRAW_PRUNE), s_off, seed, codes, p_e};
    return run_elim(h, B, e_off, e_vars, e_codes, P);
}

int run_map_body(mibn_t *h, uint32_t flags, int64_t B, const int64_t *m_off, const int32_t *m_vars, const int64_t *e_off, const int32_t *e_vars,
                 const int32_t *e_codes, int32_t *codes, double *log_p) {
    if (!h || B < 0 || !m_off || !e_off || (B && !log_p)) return MIBN_E_ARG;
    if (int rc = check_state(h, kNeedDevice | kNeedNet)) return rc;
    if (flags & ~(uint32_t)MIBN_MAP_PRUNE) { h->err = "map: unknown flag"; return MIBN_E_ARG; }
    for (int64_t b = 0; b < B; ++b)
        if (m_off[b + 1] < m_off[b] || m_off[b] < 0) { h->err = "map: m_off must be non-negative and ascending"; return MIBN_E_ARG; }
    if (B && m_off[B] > m_off[0] && (!codes || !m_vars)) return MIBN_E_ARG;
    MapPayload P{!(flags & MIBN_MAP_PRUNE), B, m_off, m_vars, codes, log_p};
    return run_elim(h, B, e_off, e_vars, e_codes, P);
}

}  // namespace

// ---------------------------------------------------------------------------------------------- likelihood findings
// mibn_set_likelihoods stages a block for the NEXT batch call.  The calls that consume it (mibn_query_batch, mibn_query_batch_ex,
// mibn_mpe_batch, mibn_map_batch, mibn_bp_batch, mibn_bp_mpe_batch, mibn_bp_evidence_batch) take it for their duration - h->lh, null for a block without a single finding: such a call is the call
// without a block, bit for bit -; the others refuse it.  Either way it is gone when the call returns, whatever the call returns.
namespace {
void drop_findings(mibn_ctx *h) {
    h->lh = nullptr;
    h->has_staged = false;
    h->staged = Findings{};
}
struct TakeFindings {
    mibn_ctx *h;
    explicit TakeFindings(mibn_ctx *h_) : h(h_) {}
    ~TakeFindings() { if (h) drop_findings(h); }
    int take(int64_t B) {
        if (!h || !h->has_staged) return MIBN_OK;
        if (h->staged.B != B) {
            h->err = "likelihood findings were set for " + std::to_string(h->staged.B) + " requests, the call has " + std::to_string(B);
            return MIBN_E_ARG;
        }
        if (h->staged.any()) h->lh = &h->staged;
        return MIBN_OK;
    }
};
int refuse_findings(mibn_ctx *h, int code, const char *call) {
    if (!h || !h->has_staged) return MIBN_OK;
    drop_findings(h);
    h->err = std::string(call) + " does not take likelihood findings: the block of mibn_set_likelihoods was dropped";
    return code;
}
}  // namespace

extern "C" int mibn_set_likelihoods(mibn_t *h, int64_t B, const int64_t *l_off, const int32_t *l_vars, const int64_t *v_off, const double *values) {
    if (!h) return MIBN_E_ARG;
    drop_findings(h);
    if (B < 0 || (B && !l_off)) { h->err = "likelihood findings: B < 0 or l_off missing"; return MIBN_E_ARG; }
    if (int rc = check_state(h, kNeedNet)) return rc;
    const Network &net = h->net;
    Findings F;
    F.B = B;
    F.l_off.assign((size_t)B + 1, 0);
    const int64_t base = B ? l_off[0] : 0;
    for (int64_t b = 0; b < B; ++b) {
        if (l_off[b + 1] < l_off[b]) { h->err = "request " + std::to_string(b) + ": l_off must be ascending"; return MIBN_E_ARG; }
        F.l_off[(size_t)b + 1] = l_off[b + 1] - base;
    }
    const int64_t n = F.l_off[(size_t)B];
    if (n && (!l_vars || !v_off || !values)) { h->err = "likelihood findings: l_vars, v_off or values missing"; return MIBN_E_ARG; }
    F.l_vars.reserve((size_t)n);
    F.v_off.assign((size_t)n + 1, 0);
    std::vector<char> seen((size_t)net.n_vars, 0);
    for (int64_t b = 0; b < B; ++b) {
        const std::string where = "request " + std::to_string(b) + ": ";
        for (int64_t k = F.l_off[(size_t)b]; k < F.l_off[(size_t)b + 1]; ++k) {
            const int32_t v = l_vars[base + k];
            if (v < 0 || v >= net.n_vars) { h->err = where + "unknown likelihood variable id " + std::to_string(v); return MIBN_E_ARG; }
            if (seen[(size_t)v]) { h->err = where + "duplicate likelihood variable id " + std::to_string(v); return MIBN_E_ARG; }
            seen[(size_t)v] = 1;
            const int64_t v0 = v_off[base + k], v1 = v_off[base + k + 1];
            if (v1 - v0 != net.card[v]) {
                h->err = where + "the finding on variable " + std::to_string(v) + " has " + std::to_string(v1 - v0) + " weights, the variable " + std::to_string(net.card[v]) + " states";
                return MIBN_E_ARG;
            }
            for (int64_t c = v0; c < v1; ++c) {
                const double x = values[c];
                if (!(x >= 0.0) || x > std::numeric_limits<double>::max()) { h->err = where + "the weights of a finding must be finite and non-negative (variable " + std::to_string(v) + ")"; return MIBN_E_ARG; }
                F.values.push_back(x);
            }
            F.l_vars.push_back(v);
            F.v_off[(size_t)k + 1] = (int64_t)F.values.size();
        }
        for (int64_t k = F.l_off[(size_t)b]; k < F.l_off[(size_t)b + 1]; ++k) seen[(size_t)l_vars[base + k]] = 0;
    }
    h->staged = std::move(F);
    h->has_staged = true;
    return MIBN_OK;
}

// (nothing of a blocking call may still run on the main stream when the caller sees its error)
extern "C" int mibn_mpe_batch(mibn_t *h, int64_t B, const int64_t *e_off, const int32_t *e_vars, const int32_t *e_codes, int32_t *codes,
                              double *log_p) {
    TakeFindings lh(h);
    if (int rc = lh.take(B)) return rc;
    return drained_on_error(h, run_mpe_body(h, B, e_off, e_vars, e_codes, codes, log_p), drain_main_unchecked);
}

extern "C" int mibn_map_batch(mibn_t *h, uint32_t flags, int64_t B, const int64_t *m_off, const int32_t *m_vars, const int64_t *e_off,
                              const int32_t *e_vars, const int32_t *e_codes, int32_t *codes, double *log_p) {
    TakeFindings lh(h);
    if (int rc = lh.take(B)) return rc;
    return drained_on_error(h, run_map_body(h, flags, B, m_off, m_vars, e_off, e_vars, e_codes, codes, log_p), drain_main_unchecked);
}

extern "C" int mibn_posterior_sample_batch(mibn_t *h, int64_t B, const int64_t *e_off, const int32_t *e_vars, const int32_t *e_codes,
                                           const int64_t *s_off, uint64_t seed, uint32_t flags, int32_t *codes, double *p_e) {
    if (int rc = refuse_findings(h, MIBN_E_ARG, "mibn_posterior_sample_batch")) return rc;
    return drained_on_error(h, run_draw_body(h, B, e_off, e_vars, e_codes, s_off, seed, flags, codes, p_e), drain_main_unchecked);
}

extern "C" int mibn_query_batch(mibn_t *h, int64_t B, const int64_t *q_off, const int32_t *q_vars,
                                const int64_t *e_off, const int32_t *e_vars, const int32_t *e_codes,
                                const int64_t *out_off, double *out) {
    TakeFindings lh(h);
    if (h && check_state(h, kNeedIdle)) return MIBN_E_STATE;
    if (int rc = lh.take(B)) return rc;
    return run_batch(h, 0, B, q_off, q_vars, e_off, e_vars, e_codes, out_off, out, nullptr);
}

extern "C" int mibn_query_batch_ex(mibn_t *h, uint32_t flags, int64_t B, const int64_t *q_off, const int32_t *q_vars,
                                   const int64_t *e_off, const int32_t *e_vars, const int32_t *e_codes,
                                   const int64_t *out_off, double *out) {
    TakeFindings lh(h);
    if (h && check_state(h, kNeedIdle)) return MIBN_E_STATE;
    if (flags & ~(uint32_t)(MIBN_Q_NOPRUNE | MIBN_Q_UNNORMALISED)) { if (h) h->err = "unknown query flag"; return MIBN_E_ARG; }
    if (int rc = lh.take(B)) return rc;
    return run_batch(h, flags, B, q_off, q_vars, e_off, e_vars, e_codes, out_off, out, nullptr);
}

extern "C" int mibn_expect_batch(mibn_t *h, uint32_t flags, int64_t B, const int64_t *q_off, const int32_t *q_vars, const int64_t *e_off,
                                 const int32_t *e_vars, const int32_t *e_codes, const int64_t *acc_base, const int64_t *acc_stride,
                                 const double *weight, int64_t n_acc, double *acc, double *p_out) {
    if (int rc = refuse_findings(h, MIBN_E_STATE, "mibn_expect_batch")) return rc;
    if (!h || B < 0 || n_acc < 0 || !q_off || !e_off || (n_acc && !acc)) return MIBN_E_ARG;
    if (int rc = check_state(h, kNeedIdle)) return rc;
    if (flags & ~(uint32_t)(MIBN_Q_NOPRUNE | MIBN_Q_UNNORMALISED)) { h->err = "unknown query flag"; return MIBN_E_ARG; }
    if (int rc = check_state(h, kNeedDevice | kNeedNet)) return rc;
    if (B >= 0x7ffffff0) { h->err = "expect: too many requests in one call"; return MIBN_E_LIMIT; }
    flags |= MIBN_Q_UNNORMALISED;
    // everything the targets depend on is checked here, on the host, before anything is launched: the requests themselves (the query
    // path's validation), then base / strides / cardinalities against [0, n_acc)
    std::vector<int64_t> out_off((size_t)B + 1, 0);
    for (int64_t b = 0; b < B; ++b) {
        Request rq;
        rq.nq = (int32_t)(q_off[b + 1] - q_off[b]);
        rq.qvars = q_vars + q_off[b];
        rq.ne = (int32_t)(e_off[b + 1] - e_off[b]);
        rq.evars = e_vars + e_off[b];
        rq.kind = ProgramKind::Raw;
        if (rq.nq < 0 || rq.ne < 0 || !request_is_valid(h->net, rq)) { h->err = "request " + std::to_string(b) + ": " + (rq.nq < 0 || rq.ne < 0 ? std::string("negative count") : validate_request(h->net, rq)); return MIBN_E_ARG; }
        if (rq.nq && (!acc_base || !acc_stride)) { h->err = "expect: acc_base / acc_stride missing"; return MIBN_E_ARG; }
        int64_t cells = 1;
        for (int i = 0; i < rq.nq; ++i) {
            cells *= h->net.card[rq.qvars[i]];
            if (cells > (int64_t(1) << 30)) { h->err = "request " + std::to_string(b) + ": query table too large"; return MIBN_E_LIMIT; }
        }
        out_off[(size_t)b + 1] = out_off[(size_t)b] + cells;
    }
    mibn_ctx::Expect &X = h->ex;
    int rc = expect_plan(B, q_off, q_vars, h->net.card.data(), out_off.data(), acc_base, acc_stride, n_acc, X.plan, h->err);
    if (rc != MIBN_OK) return rc;
    X.weight = weight;
    X.B = B;
    X.n_acc = n_acc;
    X.acc = acc;
    X.p_out = p_out;
    h->expect = true;
    rc = run_batch(h, flags, B, q_off, q_vars, e_off, e_vars, e_codes, out_off.data(), nullptr, nullptr);
    h->expect = false;
    if (rc != MIBN_OK) return rc;
    // P(e) of empty evidence with pruning: the empty product (see the query path) - the planned kernels leave its cell zero
    if (p_out && h->net.prune && !(flags & MIBN_Q_NOPRUNE))
        for (int64_t b = 0; b < B; ++b)
            if (q_off[b + 1] == q_off[b] && e_off[b + 1] == e_off[b]) p_out[b] = 1.0;
    return MIBN_OK;
}

extern "C" int mibn_submit_batch(mibn_t *h, int64_t B, const int64_t *q_off, const int32_t *q_vars,
                                 const int64_t *e_off, const int32_t *e_vars, const int32_t *e_codes,
                                 const int64_t *out_off, double *out, int32_t *ticket) {
    if (int rc = refuse_findings(h, MIBN_E_STATE, "mibn_submit_batch")) return rc;
    if (!ticket) return MIBN_E_ARG;
    return run_batch(h, 0, B, q_off, q_vars, e_off, e_vars, e_codes, out_off, out, ticket);
}

extern "C" int mibn_wait(mibn_t *h, int32_t ticket) {
    if (!h || ticket < 0 || ticket > 1) return MIBN_E_ARG;
    mibn_ctx::Pending &pd = h->pend[ticket];
    if (!pd.active) return MIBN_OK;  // (an empty batch, or already collected)
    HIP_TRY(h, hipSetDevice(h->device));
    const double t0 = now_ms();
    HIP_TRY(h, hipEventSynchronize(pd.done));
    std::memcpy(pd.out, h->res_stage[ticket].get(), pd.cells * 8);
    pd.active = false;
    h->stats.d2h_ms += now_ms() - t0;
    h->total.d2h_ms += now_ms() - t0;
    return MIBN_OK;
}

extern "C" int mibn_drain(mibn_t *h) {
    if (!h) return MIBN_E_ARG;
    if (h->planner_only) return MIBN_OK;
    HIP_TRY(h, hipSetDevice(h->device));
    return retire_all(h);
}

extern "C" int mibn_total_stats(const mibn_t *h, mibn_stats *out) {
    if (!h || !out) return MIBN_E_ARG;
    *out = h->total;
    return MIBN_OK;
}

extern "C" int mibn_total_kernel_stats(const mibn_t *h, int32_t cap, mibn_kernel_stat *out, int32_t *n) {
    if (!h || !out || !n) return MIBN_E_ARG;
    int k = 0;
    for (int i = 0; i < kStatSlots && k < cap; ++i)
        if (h->ktotal[i].launches > 0) out[k++] = h->ktotal[i];
    *n = k;
    return MIBN_OK;
}

extern "C" int mibn_last_kernel_stats(const mibn_t *h, int32_t cap, mibn_kernel_stat *out, int32_t *n) {
    if (!h || !out || !n) return MIBN_E_ARG;
    int k = 0;
    for (int i = 0; i < kStatSlots && k < cap; ++i)
        if (h->kstats[i].launches > 0) out[k++] = h->kstats[i];
    *n = k;
    return MIBN_OK;
}

extern "C" int mibn_gibbs(mibn_t *h, int32_t n_q, const int32_t *q_vars, int32_t n_e, const int32_t *e_vars,
                          const int32_t *e_codes, const int32_t *cycle, int64_t n_chains, int64_t n_iterations,
                          uint64_t seed, int64_t *counts) {
    return mibn_gibbs_shard(h, n_q, q_vars, n_e, e_vars, e_codes, cycle, 0, n_chains, n_iterations, seed, counts);
}

extern "C" int mibn_gibbs_shard(mibn_t *h, int32_t n_q, const int32_t *q_vars, int32_t n_e, const int32_t *e_vars,
                                const int32_t *e_codes, const int32_t *cycle, int64_t chain_first, int64_t n_chains,
                                int64_t n_iterations, uint64_t seed, int64_t *counts) {
    if (!h || !q_vars || !counts || n_chains < 0 || chain_first < 0 || n_iterations < 0) return MIBN_E_ARG;
    if (int rc = check_state(h, kNeedDevice | kNeedNet)) return rc;
    Request rq;
    rq.nq = n_q; rq.qvars = q_vars; rq.ne = n_e; rq.evars = e_vars;
    std::string e = validate_request(h->net, rq);
    if (!e.empty()) { h->err = e; return MIBN_E_ARG; }
    if (n_chains == 0) return zero_histogram(h->net, n_q, q_vars, kGibbsTooLarge, counts, h->err);  // an empty shard (more ranks than chains)
    HIP_TRY(h, hipSetDevice(h->device));
    return gibbs_run(h->net, h->d_pool, h->stream, h->gibbs_lds, n_q, q_vars, n_e, e_vars, e_codes, cycle, chain_first, n_chains,
                     n_iterations, seed, counts, h->err, h->stats.kernel_ms);
}

extern "C" int mibn_gibbs_conditional(mibn_t *h, int32_t n_e, const int32_t *e_vars, const int32_t *e_codes, const int32_t *cycle,
                                      int32_t var, int64_t n_rows, const uint8_t *states, double *out) {
    if (!h || n_rows < 0 || (n_rows && (!states || !out)) || (n_e && (!e_vars || !e_codes))) return MIBN_E_ARG;
    if (int rc = check_state(h, kNeedDevice | kNeedNet)) return rc;
    if (var < 0 || var >= h->net.n_vars) { h->err = "gibbs conditional: unknown variable"; return MIBN_E_ARG; }
    Request rq;
    rq.ne = n_e; rq.evars = e_vars;
    std::string e = validate_mpe_request(h->net, rq);  // unknown or duplicate evidence ids
    if (!e.empty()) { h->err = e; return MIBN_E_ARG; }
    for (int64_t r = 0; r < n_rows; ++r)
        for (int v = 0; v < h->net.n_vars; ++v)
            if (states[r * h->net.n_vars + v] >= h->net.card[v]) { h->err = "gibbs conditional: a state code is outside its variable's domain"; return MIBN_E_ARG; }
    if (n_rows == 0) return MIBN_OK;
    HIP_TRY(h, hipSetDevice(h->device));
    const int32_t q0 = var;  // (the histogram of the ordinary launch: one variable, unused)
    double ms = 0;
    return gibbs_run(h->net, h->d_pool, h->stream, h->gibbs_lds, 1, &q0, n_e, e_vars, e_codes, cycle, 0, n_rows, 1, 0, nullptr, h->err, ms,
                     var, states, out);
}

// ---------------------------------------------------------------------------------------------- loopy belief propagation
// mibn_bp_batch: plan (bp_plan.h), upload the records once, then launch by launch - at most `chunk` requests, in the global form as
// many as have slabs in the arena of lane 0 - upload the evidence, run bp_kernel, download.  Blocking, on the main stream, buffers of
// its own; last-call statistics only, nothing a later call reads.  mibn_bp_mpe_batch (`mx`) is the same call around bp_max_kernel:
// the larger state, the colouring next to the records, codes / log_p / info in place of the beliefs.  mibn_bp_evidence_batch (`evd`)
// is the same call around bp_evidence_kernel: its own state, log_z beside the beliefs, and - where the caller wants family beliefs
// or expected counts - one family-belief row per request of the launch, in the arena behind the slabs, which bp_accumulate_kernel adds into
// `acc` after every launch; `acc` stays on the device between the launches.
namespace {
struct BpEvOut {
    const double *weight;  // or null
    double *log_z;
    double *fbeliefs;      // or null
    int64_t n_acc;
    double *acc;           // or null
};
struct BpMpeOut {
    int32_t polish_sweeps;
    int32_t *codes;
    double *log_p;
    int32_t *info;  // or null
};
int bp_body(mibn_ctx *h, int64_t B, const int64_t *e_off, const int32_t *e_vars, const int32_t *e_codes, int32_t max_iterations, double tol,
            double damping, double *beliefs, int32_t *iterations, double *residual, const BpMpeOut *mx = nullptr, const BpEvOut *evd = nullptr) {
    const double t_start = now_ms();
    reset_last_stats(h);
    const Network &net = h->net;
    int rc;
    if ((rc = mx ? bp_mpe_check_args(max_iterations, tol, damping, mx->polish_sweeps, h->err) : bp_check_args(max_iterations, tol, damping, h->err))) return rc;
    const Findings *F = h->lh;
    for (int64_t b = 0; b < B; ++b) {
        if (e_off[b + 1] < e_off[b] || e_off[b] < 0) { h->err = "request " + std::to_string(b) + ": e_off must be non-negative and ascending"; return MIBN_E_ARG; }
        Request rq;
        rq.ne = (int32_t)(e_off[b + 1] - e_off[b]);
        if (rq.ne && (!e_vars || !e_codes)) { h->err = "bp: e_vars or e_codes missing"; return MIBN_E_ARG; }
        rq.evars = rq.ne ? e_vars + e_off[b] : nullptr;
        if (F) { rq.nl = (int32_t)(F->l_off[(size_t)b + 1] - F->l_off[(size_t)b]); rq.lvars = F->l_vars.data() + F->l_off[(size_t)b]; }
        const std::string e = validate_mpe_request(net, rq);  // unknown or duplicate evidence ids, a finding variable that is evidence
        if (!e.empty()) { h->err = "request " + std::to_string(b) + ": " + e; return MIBN_E_ARG; }
    }
    BpMpePlan M;
    BpEvPlan E;
    BpPlan &P = evd ? E.bp : M.bp;
    if ((rc = mx ? bp_mpe_plan(net, h->bp_lds, M, h->err) : evd ? bp_ev_plan(net, h->bp_lds, E, h->err) : bp_plan(net, h->bp_lds, P, h->err))) return rc;
    if (evd && (rc = bp_ev_check_acc(E, evd->acc != nullptr, evd->n_acc, evd->weight, B, h->err))) return rc;
    const BpForm form = mx ? M.form : evd ? E.form : P.form;
    const size_t slab_bytes = mx ? M.slab_bytes : evd ? E.slab_bytes : P.slab_bytes;
    const bool rows = evd && (evd->fbeliefs || evd->acc);  // family-belief rows on the device
    const size_t fc = evd ? (size_t)E.fcells : 0;
    if (B == 0) return MIBN_OK;
    HIP_TRY(h, hipSetDevice(h->device));
    if ((rc = drain_streams(h))) return rc;  // (the arena of lane 0 is the query calls' too)
    const hipStream_t S = h->stream;
    size_t free_b = 0, total_b = 0;
    HIP_TRY(h, hipMemGetInfo(&free_b, &total_b));
    const double budget = std::min(h->arena_gb * 1e9, 0.8 * (double)(free_b + h->d_arena[0].cap()));
    const int64_t per_launch = evd ? bp_ev_launch_requests(E, rows, h->chunk, budget) : bp_launch_requests(form, slab_bytes, h->chunk, budget);
    if (per_launch < 1) { h->err = "bp: one request's messages need " + std::to_string((double)(slab_bytes + (rows ? 8 * fc : 0)) / 1e9) + " GB, above the arena budget"; return MIBN_E_NOMEM; }
    const int64_t n_max = std::min(B, per_launch);
    const size_t lam = (size_t)P.lam_cells, nv = (size_t)net.n_vars;
    DevBuf<BpEdge> d_edges;
    DevBuf<BpVar> d_vars;
    DevBuf<int32_t> d_nbr, d_ev, d_ec, d_lv, d_it, d_nbre, d_coff, d_cmem, d_codes, d_info;
    DevBuf<int64_t> d_eoff, d_loff, d_voff;
    DevBuf<double> d_val, d_bel, d_res, d_logp, d_acc, d_w;
    DevBuf<int32_t> d_foff;
    std::vector<int32_t> info_host;  // (a caller without `info`)
    Event ev0, ev1, ev2;
    HIP_TRY(h, d_edges.reset(P.edges.size()));
    HIP_TRY(h, d_vars.reset(P.vars.size()));
    HIP_TRY(h, d_nbr.reset(P.nbr_moff.size()));
    HIP_TRY(h, d_eoff.reset((size_t)n_max + 1));
    if (!mx && beliefs) HIP_TRY(h, d_bel.reset((size_t)n_max * lam));
    if (evd) {
        HIP_TRY(h, d_foff.reset(E.foff.size()));
        HIP_TRY(h, d_logp.reset((size_t)n_max));
        if (evd->acc) HIP_TRY(h, d_acc.reset(std::max<size_t>(1, fc)));
        if (evd->acc && evd->weight) HIP_TRY(h, d_w.reset((size_t)n_max));
    }
    if (mx) {
        HIP_TRY(h, d_nbre.reset(P.nbr.size()));
        HIP_TRY(h, d_coff.reset(M.col.off.size()));
        HIP_TRY(h, d_cmem.reset(M.col.members.size()));
        HIP_TRY(h, d_codes.reset((size_t)n_max * nv));
        HIP_TRY(h, d_logp.reset((size_t)n_max));
        HIP_TRY(h, d_info.reset((size_t)n_max * 3));
        if (!mx->info) info_host.resize((size_t)n_max * 3);
    }
    HIP_TRY(h, d_it.reset((size_t)n_max));
    HIP_TRY(h, d_res.reset((size_t)n_max));
    HIP_TRY(h, ev0.ensure());
    HIP_TRY(h, ev1.ensure());
    HIP_TRY(h, ev2.ensure());
    HIP_TRY(h, hipMemcpyAsync(d_edges, P.edges.data(), P.edges.size() * sizeof(BpEdge), hipMemcpyHostToDevice, S));
    HIP_TRY(h, hipMemcpyAsync(d_vars, P.vars.data(), P.vars.size() * sizeof(BpVar), hipMemcpyHostToDevice, S));
    HIP_TRY(h, hipMemcpyAsync(d_nbr, P.nbr_moff.data(), P.nbr_moff.size() * 4, hipMemcpyHostToDevice, S));
    if (mx) {
        HIP_TRY(h, hipMemcpyAsync(d_nbre, P.nbr.data(), P.nbr.size() * 4, hipMemcpyHostToDevice, S));
        HIP_TRY(h, hipMemcpyAsync(d_coff, M.col.off.data(), M.col.off.size() * 4, hipMemcpyHostToDevice, S));
        HIP_TRY(h, hipMemcpyAsync(d_cmem, M.col.members.data(), M.col.members.size() * 4, hipMemcpyHostToDevice, S));
    }
    if (evd) {
        HIP_TRY(h, hipMemcpyAsync(d_foff, E.foff.data(), E.foff.size() * 4, hipMemcpyHostToDevice, S));
        if (evd->acc && fc) HIP_TRY(h, hipMemcpyAsync(d_acc, evd->acc, fc * 8, hipMemcpyHostToDevice, S));
    }
    const BpKernel kernel = bp_kernel_of(form);
    const BpMaxKernel max_kernel = bp_max_kernel_of(form);
    const BpEvKernel ev_kernel = bp_evidence_kernel_of(form);
    const size_t lds = mx ? bp_lds_bytes(M) : evd ? bp_lds_bytes(E) : bp_lds_bytes(P);
    if (lds > 64 * 1024)
        HIP_TRY(h, hipFuncSetAttribute(mx ? (const void *)max_kernel : evd ? (const void *)ev_kernel : (const void *)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    // the arena of lane 0: the slabs of the launch's requests (MsgGlobal), then their family-belief rows - both inside the budget the
    // launch size was cut to, and kept from call to call
    const size_t slabs_total = form == BpForm::MsgGlobal ? (size_t)n_max * slab_bytes : 0, rows_total = rows ? (size_t)n_max * fc * 8 : 0;
    if (slabs_total + rows_total != 0 && (rc =grow_arena(h, 0, slabs_total + rows_total, (int64_t)(budget / 8.0), S))) return rc;
    BpMaxArgs MA{};
    BpEvArgs EA{};
    BpArgs &A = evd ? EA.bp : MA.bp;
    A.pool = h->d_pool;
    A.edges = d_edges;
    A.vars = d_vars;
    A.nbr_moff = d_nbr;
    A.slabs = reinterpret_cast<unsigned char *>(h->d_arena[0].get());
    double *const d_fb = rows_total ? reinterpret_cast<double *>(A.slabs + slabs_total) : nullptr;
    A.slab_bytes = slab_bytes;
    A.n_vars = net.n_vars;
    A.n_edges = (int32_t)P.edges.size();
    A.cells = P.cells;
    A.lam_cells = P.lam_cells;
    A.max_iterations = max_iterations;
    A.tol = tol;
    A.damping = damping;
    if (mx) {
        MA.nbr = d_nbre;
        MA.col_off = d_coff;
        MA.col_members = d_cmem;
        MA.n_colours = M.col.n_colours;
        MA.polish_sweeps = mx->polish_sweeps;
        MA.codes = d_codes;
        MA.log_p = d_logp;
        MA.info = d_info;
    }
    if (evd) {
        EA.foff = d_foff;
        EA.fcells = E.fcells;
        EA.log_z = d_logp;
        EA.fbeliefs = d_fb;
    }
    const double req_bytes = evd ? 8.0 * (double)fc : 0.0;  // (the final phase: one more pass over the CPT cells)
    std::vector<int64_t> off;
    for (int64_t b0 = 0; b0 < B; b0 += n_max) {
        const int64_t n = std::min(n_max, B - b0);
        double t0 = now_ms();
        off.assign((size_t)n + 1, 0);
        for (int64_t r = 0; r <= n; ++r) off[(size_t)r] = e_off[b0 + r] - e_off[b0];
        const size_t ne = (size_t)off[(size_t)n];
        HIP_TRY(h, d_ev.ensure(std::max<size_t>(1, ne)));
        HIP_TRY(h, d_ec.ensure(std::max<size_t>(1, ne)));
        HIP_TRY(h, hipMemcpyAsync(d_eoff, off.data(), ((size_t)n + 1) * 8, hipMemcpyHostToDevice, S));
        if (ne) {
            HIP_TRY(h, hipMemcpyAsync(d_ev, e_vars + e_off[b0], ne * 4, hipMemcpyHostToDevice, S));
            HIP_TRY(h, hipMemcpyAsync(d_ec, e_codes + e_off[b0], ne * 4, hipMemcpyHostToDevice, S));
        }
        HIP_TRY(h, hipStreamSynchronize(S));  // (`off` is reused below)
        A.e_off = d_eoff;
        A.e_vars = d_ev;
        A.e_codes = d_ec;
        A.l_off = nullptr;
        if (F) {  // the findings of requests [b0, b0 + n), offsets relative to the launch
            const size_t k0 = (size_t)F->l_off[(size_t)b0], k1 = (size_t)F->l_off[(size_t)(b0 + n)], nk = k1 - k0;
            const size_t w0 = (size_t)F->v_off[k0], nw = (size_t)F->v_off[k1] - w0;
            std::vector<int64_t> lo((size_t)n + 1), vo(nk + 1);
            for (int64_t r = 0; r <= n; ++r) lo[(size_t)r] = F->l_off[(size_t)(b0 + r)] - (int64_t)k0;
            for (size_t k = 0; k <= nk; ++k) vo[k] = F->v_off[k0 + k] - (int64_t)w0;
            HIP_TRY(h, d_loff.ensure((size_t)n + 1));
            HIP_TRY(h, d_voff.ensure(nk + 1));
            HIP_TRY(h, d_lv.ensure(std::max<size_t>(1, nk)));
            HIP_TRY(h, d_val.ensure(std::max<size_t>(1, nw)));
            HIP_TRY(h, hipMemcpyAsync(d_loff, lo.data(), lo.size() * 8, hipMemcpyHostToDevice, S));
            HIP_TRY(h, hipMemcpyAsync(d_voff, vo.data(), vo.size() * 8, hipMemcpyHostToDevice, S));
            if (nk) HIP_TRY(h, hipMemcpyAsync(d_lv, F->l_vars.data() + k0, nk * 4, hipMemcpyHostToDevice, S));
            if (nw) HIP_TRY(h, hipMemcpyAsync(d_val, F->values.data() + w0, nw * 8, hipMemcpyHostToDevice, S));
            HIP_TRY(h, hipStreamSynchronize(S));  // (lo and vo leave scope)
            A.l_off = d_loff;
            A.l_vars = d_lv;
            A.v_off = d_voff;
            A.values = d_val;
        }
        h->stats.h2d_ms += now_ms() - t0;
        if (evd && evd->acc && evd->weight) HIP_TRY(h, hipMemcpyAsync(d_w, evd->weight + b0, (size_t)n * 8, hipMemcpyHostToDevice, S));
        A.beliefs = mx || !beliefs ? nullptr : d_bel.get();
        A.iterations = d_it;
        A.residual = d_res;
        HIP_TRY(h, hipEventRecord(ev0, S));
        if (mx) hipLaunchKernelGGL(max_kernel, dim3((unsigned)n), dim3((unsigned)P.threads), lds, S, MA);
        else if (evd) hipLaunchKernelGGL(ev_kernel, dim3((unsigned)n), dim3((unsigned)P.threads), lds, S, EA);
        else hipLaunchKernelGGL(kernel, dim3((unsigned)n), dim3((unsigned)P.threads), lds, S, A);
        HIP_TRY(h, hipGetLastError());
        HIP_TRY(h, hipEventRecord(ev1, S));
        if (evd && evd->acc && fc) {
            hipLaunchKernelGGL(bp_accumulate_kernel, dim3((unsigned)((fc + 255) / 256)), dim3(256), 0, S, d_acc.get(), (const double *)d_fb,
                               evd->weight ? (const double *)d_w.get() : nullptr, n, E.fcells);
            HIP_TRY(h, hipGetLastError());
            HIP_TRY(h, hipEventRecord(ev2, S));
        }
        t0 = now_ms();
        if (mx) {
            HIP_TRY(h, hipMemcpyAsync(mx->codes + (size_t)b0 * nv, d_codes, (size_t)n * nv * 4, hipMemcpyDeviceToHost, S));
            HIP_TRY(h, hipMemcpyAsync(mx->log_p + b0, d_logp, (size_t)n * 8, hipMemcpyDeviceToHost, S));
            HIP_TRY(h, hipMemcpyAsync(mx->info ? mx->info + (size_t)b0 * 3 : info_host.data(), d_info, (size_t)n * 12, hipMemcpyDeviceToHost, S));
        } else if (beliefs)
            HIP_TRY(h, hipMemcpyAsync(beliefs + (size_t)b0 * lam, d_bel, (size_t)n * lam * 8, hipMemcpyDeviceToHost, S));
        if (evd) {
            HIP_TRY(h, hipMemcpyAsync(evd->log_z + b0, d_logp, (size_t)n * 8, hipMemcpyDeviceToHost, S));
            if (evd->fbeliefs && fc) HIP_TRY(h, hipMemcpyAsync(evd->fbeliefs + (size_t)b0 * fc, d_fb, (size_t)n * fc * 8, hipMemcpyDeviceToHost, S));
        }
        HIP_TRY(h, hipMemcpyAsync(iterations + b0, d_it, (size_t)n * 4, hipMemcpyDeviceToHost, S));
        HIP_TRY(h, hipMemcpyAsync(residual + b0, d_res, (size_t)n * 8, hipMemcpyDeviceToHost, S));
        HIP_TRY(h, hipStreamSynchronize(S));
        h->stats.d2h_ms += now_ms() - t0;
        float ms = 0;
        HIP_TRY(h, hipEventElapsedTime(&ms, ev0, ev1));
        double iters = 0;
        for (int64_t r = 0; r < n; ++r) iters += iterations[b0 + r];
        const double bytes = P.iter_bytes * iters + req_bytes * (double)n;
        book_stat(h, mx ? kStatBpMax : evd ? kStatBpEvidence : kStatBp, 1, ms, bytes, (double)n, true, false);
        h->stats.kernel_ms += ms;
        h->stats.n_launches += 1;
        h->stats.n_workgroups += (double)n;
        h->stats.alg_bytes += bytes;
        if (evd && evd->acc && fc) {  // reads the launch's rows, reads and writes acc
            HIP_TRY(h, hipEventElapsedTime(&ms, ev1, ev2));
            book_stat(h, kStatBpAccumulate, 1, ms, 8.0 * (double)fc * (double)(n + 2), (double)n, true, false);
            h->stats.kernel_ms += ms;
            h->stats.n_launches += 1;
        }
    }
    if (evd && evd->acc && fc) {
        HIP_TRY(h, hipMemcpyAsync(evd->acc, d_acc, fc * 8, hipMemcpyDeviceToHost, S));
        HIP_TRY(h, hipStreamSynchronize(S));
    }
    if (form == BpForm::MsgGlobal) h->stats.arena_bytes = (double)n_max * (double)slab_bytes;
    h->stats.total_ms = now_ms() - t_start;
    return MIBN_OK;
}
}  // namespace

extern "C" int mibn_bp_evidence_batch(mibn_t *h, int64_t B, const int64_t *e_off, const int32_t *e_vars, const int32_t *e_codes,
                                      int32_t max_iterations, double tol, double damping, const double *weight, double *log_z, double *beliefs,
                                      double *fbeliefs, int64_t n_acc, double *acc, int32_t *iterations, double *residual) {
    TakeFindings lh(h);
    if (!h || B < 0 || (B && (!e_off || !log_z || !iterations || !residual))) return MIBN_E_ARG;
    if (int rc = check_state(h, kNeedIdle)) return rc;
    if (int rc = check_state(h, kNeedDevice | kNeedNet)) return rc;
    if (int rc = lh.take(B)) return rc;
    const BpEvOut evd{weight, log_z, fbeliefs, n_acc, acc};
    return drained_on_error(h, bp_body(h, B, e_off, e_vars, e_codes, max_iterations, tol, damping, beliefs, iterations, residual, nullptr, &evd), drain_main_unchecked);
}

extern "C" int mibn_bp_batch(mibn_t *h, int64_t B, const int64_t *e_off, const int32_t *e_vars, const int32_t *e_codes, int32_t max_iterations,
                             double tol, double damping, double *beliefs, int32_t *iterations, double *residual) {
    TakeFindings lh(h);
    if (!h || B < 0 || (B && (!e_off || !beliefs || !iterations || !residual))) return MIBN_E_ARG;
    if (int rc = check_state(h, kNeedIdle)) return rc;
    if (int rc = check_state(h, kNeedDevice | kNeedNet)) return rc;
    if (int rc = lh.take(B)) return rc;
    return drained_on_error(h, bp_body(h, B, e_off, e_vars, e_codes, max_iterations, tol, damping, beliefs, iterations, residual), drain_main_unchecked);
}

extern "C" int mibn_bp_mpe_batch(mibn_t *h, int64_t B, const int64_t *e_off, const int32_t *e_vars, const int32_t *e_codes, int32_t max_iterations,
                                 double tol, double damping, int32_t polish_sweeps, int32_t *codes, double *log_p, int32_t *iterations,
                                 double *residual, int32_t *info) {
    TakeFindings lh(h);
    if (!h || B < 0 || (B && (!e_off || !codes || !log_p || !iterations || !residual))) return MIBN_E_ARG;
    if (int rc = check_state(h, kNeedIdle)) return rc;
    if (int rc = check_state(h, kNeedDevice | kNeedNet)) return rc;
    if (int rc = lh.take(B)) return rc;
    const BpMpeOut mx{polish_sweeps, codes, log_p, info};
    return drained_on_error(h, bp_body(h, B, e_off, e_vars, e_codes, max_iterations, tol, damping, nullptr, iterations, residual, &mx), drain_main_unchecked);
}

extern "C" int mibn_sample(mibn_t *h, int64_t n_samples, int32_t n_init, const int32_t *init_vars, const int32_t *init_codes,
                           uint64_t seed, uint8_t *states) {
    if (!h || n_samples < 0 || !states || (n_init && (!init_vars || !init_codes))) return MIBN_E_ARG;
    if (int rc = check_state(h, kNeedDevice | kNeedNet)) return rc;
    if (n_samples == 0) return MIBN_OK;
    HIP_TRY(h, hipSetDevice(h->device));
    return sample_run(h->net, h->d_pool, h->stream, kSampleMode, 0, nullptr, n_init, init_vars, init_codes, 0, nullptr, nullptr,
                      n_samples, seed, states, nullptr, nullptr, h->err);
}

extern "C" int mibn_sample_probe(mibn_t *h, int64_t n_rows, const uint8_t *states, int32_t cdf_stride, double *likelihood, double *cdf) {
    if (!h || n_rows < 0 || (n_rows && (!states || !likelihood || !cdf))) return MIBN_E_ARG;
    if (int rc = check_state(h, kNeedDevice | kNeedNet)) return rc;
    for (int v = 0; v < h->net.n_vars; ++v)
        if (h->net.card[v] > cdf_stride) { h->err = "sample probe: cdf_stride below a variable's cardinality"; return MIBN_E_ARG; }
    for (int64_t r = 0; r < n_rows; ++r)
        for (int v = 0; v < h->net.n_vars; ++v)
            if (states[r * h->net.n_vars + v] >= h->net.card[v]) { h->err = "sample probe: a state code is outside its variable's domain"; return MIBN_E_ARG; }
    if (n_rows == 0) return MIBN_OK;
    HIP_TRY(h, hipSetDevice(h->device));
    return sample_run(h->net, h->d_pool, h->stream, kProbeMode, 0, nullptr, 0, nullptr, nullptr, 0, nullptr, nullptr, n_rows, 0,
                      const_cast<uint8_t *>(states), nullptr, nullptr, h->err, cdf_stride, likelihood, cdf);
}

extern "C" int mibn_sampling_query(mibn_t *h, int32_t mode, int32_t n_q, const int32_t *q_vars, int32_t n_e, const int32_t *e_vars,
                                   const int32_t *e_codes, int64_t n_samples, uint64_t seed, double *weight_sum, int64_t *counts) {
    if (!h || !q_vars || !counts || n_samples < 0 || (mode != MIBN_REJECTION && mode != MIBN_LIKELIHOOD)) return MIBN_E_ARG;
    if (mode == MIBN_LIKELIHOOD && !weight_sum) return MIBN_E_ARG;
    if (int rc = check_state(h, kNeedDevice | kNeedNet)) return rc;
    Request rq;
    rq.nq = n_q; rq.qvars = q_vars; rq.ne = n_e; rq.evars = e_vars;
    std::string e = validate_request(h->net, rq);
    if (!e.empty()) { h->err = e; return MIBN_E_ARG; }
    HIP_TRY(h, hipSetDevice(h->device));
    if (mode == MIBN_LIKELIHOOD)  // the event is clamped (bayes_net.py:646)
        return sample_run(h->net, h->d_pool, h->stream, kLikelihoodMode, n_q, q_vars, n_e, e_vars, e_codes, 0, nullptr, nullptr,
                          n_samples, seed, nullptr, weight_sum, counts, h->err);
    // rejection: nothing is clamped, samples that disagree with the event are dropped (bayes_net.py:604-612);
    // a label outside the domain can never be drawn
    for (int i = 0; i < n_e; ++i)
        if (e_codes[i] < 0 || e_codes[i] >= h->net.card[e_vars[i]]) return zero_histogram(h->net, n_q, q_vars, kSamplingTooLarge, counts, h->err);
    return sample_run(h->net, h->d_pool, h->stream, kRejectionMode, n_q, q_vars, 0, nullptr, nullptr, n_e, e_vars, e_codes, n_samples,
                      seed, nullptr, nullptr, counts, h->err);
}

extern "C" int mibn_count_tables(mibn_t *h, int64_t n_rows, int32_t n_cols, const uint8_t *codes, int32_t row_major, const int32_t *card,
                                 int32_t n_tables, const int64_t *scope_off, const int32_t *scope_cols, const int64_t *counts_off,
                                 int64_t *counts) {
    if (!h || n_rows < 0 || n_cols < 0 || n_tables < 0 || (n_rows && n_cols && !codes) || !card || !scope_off || !scope_cols ||
        !counts_off || !counts || (row_major != 0 && row_major != 1))
        return MIBN_E_ARG;
    if (int rc = check_state(h, kNeedDevice)) return rc;
    HIP_TRY(h, hipSetDevice(h->device));
    return count_run(h->stream, n_rows, n_cols, codes, row_major != 0, card, n_tables, scope_off, scope_cols, counts_off, counts, h->err);
}

extern "C" int mibn_count_tables_w(mibn_t *h, int64_t n_rows, int32_t n_cols, const uint8_t *codes, int32_t row_major, const int32_t *card,
                                   int32_t n_tables, const int64_t *scope_off, const int32_t *scope_cols, const int64_t *counts_off,
                                   const uint32_t *weights, int64_t *counts) {
    if (!h || n_rows < 0 || n_cols < 0 || n_tables < 0 || (n_rows && n_cols && !codes) || !card || !scope_off || !scope_cols ||
        !counts_off || !counts || (n_rows && !weights) || (row_major != 0 && row_major != 1))
        return MIBN_E_ARG;
    if (int rc = check_state(h, kNeedDevice)) return rc;
    HIP_TRY(h, hipSetDevice(h->device));
    return count_run_weighted(h->stream, n_rows, n_cols, codes, row_major != 0, card, n_tables, scope_off, scope_cols, counts_off, weights, counts, h->err);
}

extern "C" int mibn_dataset_create(mibn_t *h, int64_t n_rows, int32_t n_cols, const uint8_t *codes, int32_t row_major, const int32_t *card, int32_t *id) {
    if (!h || !id || n_rows < 0 || n_cols < 0 || (n_rows && n_cols && !codes) || (n_cols && !card) || (row_major != 0 && row_major != 1)) return MIBN_E_ARG;
    *id = -1;
    if (int rc = check_state(h, kNeedDevice)) return rc;
    for (int c = 0; c < n_cols; ++c)
        if (card[c] < 1 || card[c] > 256) { h->err = "dataset: cardinality outside 1..256"; return MIBN_E_LIMIT; }
    // a code outside its column's domain would make the count kernels write outside a table: checked here, once
    {
        std::vector<uint8_t> top((size_t)n_cols, 0);
        if (row_major) {
            for (int64_t r = 0; r < n_rows; ++r) {
                const uint8_t *row = codes + r * n_cols;
                for (int c = 0; c < n_cols; ++c) top[(size_t)c] = std::max(top[(size_t)c], row[c]);
            }
        } else {
            for (int c = 0; c < n_cols; ++c) {
                const uint8_t *col = codes + (int64_t)c * n_rows;
                uint8_t m = 0;
                for (int64_t r = 0; r < n_rows; ++r) m = std::max(m, col[r]);
                top[(size_t)c] = m;
            }
        }
        for (int c = 0; c < n_cols; ++c)
            if (n_rows && (int)top[(size_t)c] >= card[c]) { h->err = "dataset: column " + std::to_string(c) + " holds a code outside its cardinality"; return MIBN_E_ARG; }
    }
    HIP_TRY(h, hipSetDevice(h->device));
    mibn_ctx::Dataset ds;
    const size_t code_bytes = (size_t)n_rows * (size_t)n_cols;
    DevBuf<uint8_t> d_rows;
    hipError_t e = ds.d_codes.reset(std::max<size_t>(16, code_bytes));
    if (e == hipSuccess && row_major && code_bytes) e = d_rows.reset(code_bytes);
    if (e == hipSuccess) e = count_upload_codes(h->stream, n_rows, n_cols, codes, row_major != 0, ds.d_codes, d_rows);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess) {
        h->err = std::string("dataset: ") + hipGetErrorString(e);
        return MIBN_E_HIP;
    }
    ds.n_rows = n_rows;
    ds.n_cols = n_cols;
    ds.card.assign(card, card + n_cols);
    ds.live = true;
    if (h->datasets.size() >= 0x7ffffff0u) { h->err = "dataset: too many data sets"; return MIBN_E_LIMIT; }
    h->datasets.push_back(std::move(ds));
    *id = (int32_t)h->datasets.size() - 1;
    return MIBN_OK;
}

extern "C" int mibn_dataset_destroy(mibn_t *h, int32_t id) {
    if (!h) return MIBN_E_ARG;
    if (id < 0 || (size_t)id >= h->datasets.size() || !h->datasets[(size_t)id].live) { h->err = "dataset: unknown or destroyed id"; return MIBN_E_ARG; }
    HIP_TRY(h, hipSetDevice(h->device));
    mibn_ctx::Dataset &ds = h->datasets[(size_t)id];
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    HIP_TRY(h, ds.d_codes.release());
    HIP_TRY(h, ds.d_weights.release());
    ds = mibn_ctx::Dataset{};
    return MIBN_OK;
}

static int tables_enter(mibn_ctx *h, int32_t id, const char *what);

static int dataset_of(mibn_ctx *h, int32_t id, const char *what, mibn_ctx::Dataset *&ds) {
    if (int rc = tables_enter(h, id, what)) return rc;
    ds = &h->datasets[(size_t)id];
    return MIBN_OK;
}

extern "C" int mibn_dataset_set_weights(mibn_t *h, int32_t id, int32_t n_sets, const uint32_t *weights) {
    if (!h || n_sets < 0) return MIBN_E_ARG;
    mibn_ctx::Dataset *ds = nullptr;
    if (int rc = dataset_of(h, id, "weights", ds)) return rc;
    if (n_sets && ds->n_rows && !weights) { h->err = "weights: no weights given"; return MIBN_E_ARG; }
    std::vector<int64_t> sums;
    if (int rc = weight_sums(weights, n_sets, ds->n_rows, sums, h->err)) return rc;
    HIP_TRY(h, hipSetDevice(h->device));
    const size_t n = (size_t)n_sets * (size_t)ds->n_rows;
    DevBuf<uint32_t> fresh;
    if (n_sets) {
        HIP_TRY(h, fresh.reset(std::max<size_t>(1, n)));
        if (n) HIP_TRY(h, hipMemcpyAsync(fresh, weights, 4 * n, hipMemcpyHostToDevice, h->stream));
    }
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    ds->d_weights = std::move(fresh);
    ds->n_sets = n_sets;
    ds->weight_sum = std::move(sums);
    return MIBN_OK;
}

extern "C" int mibn_dataset_bootstrap(mibn_t *h, int32_t id, int32_t n_sets, uint64_t seed, uint32_t *weights_out) {
    if (!h || n_sets < 0) return MIBN_E_ARG;
    mibn_ctx::Dataset *ds = nullptr;
    if (int rc = dataset_of(h, id, "bootstrap", ds)) return rc;
    if (ds->n_rows > 0xffffffffll) { h->err = "bootstrap: the data set has more than 2^32 - 1 rows"; return MIBN_E_LIMIT; }
    HIP_TRY(h, hipSetDevice(h->device));
    const size_t n = (size_t)n_sets * (size_t)ds->n_rows;
    DevBuf<uint32_t> fresh;
    if (n_sets) {
        HIP_TRY(h, fresh.reset(std::max<size_t>(1, n)));
        HIP_TRY(h, bootstrap_weights_launch(h->stream, fresh, ds->n_rows, n_sets, seed));
        if (n && weights_out) HIP_TRY(h, hipMemcpyAsync(weights_out, fresh, 4 * n, hipMemcpyDeviceToHost, h->stream));
    }
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    ds->d_weights = std::move(fresh);
    ds->n_sets = n_sets;
    ds->weight_sum.assign((size_t)n_sets, ds->n_rows);
    return MIBN_OK;
}

// ---- what mibn_score_families and mibn_ci_tests share: a batch of tables over a resident data set, checked and packed on the host,
// counted sub-batch by sub-batch into one buffer and reduced there by the caller's kernels; three events per sub-batch
struct TableSub {
    int f0 = 0, f1 = 0;           // tables of the call
    int64_t cells = 0;
    std::vector<int64_t> off;     // first cell of every table in the count buffer (a sub-batch starts at cell 0), then the end
    CountPack pack;
    CountWeightsPack wpack;       // (weighted calls: where the weight-set arrays lie in pack.i32)
    size_t o_i32 = 0, o_i64 = 0;  // the pack in the metadata buffer
    double count_launches = 0, reduce_launches = 0, reduce_bytes = 0;
};

struct TableBatch {
    std::vector<int64_t> cells_of;
    std::vector<TableSub> subs;
    std::vector<char> meta;  // everything the kernels read but the counts: ONE upload per call
    int64_t max_cells = 1;
    const int32_t *wset = nullptr;  // mibn_score_families_w / mibn_ci_tests_w: the weight set of every table, checked; else NULL
    // N of table f: W_s of its set, n_rows without one
    int64_t rows_of(const mibn_ctx::Dataset &ds, int f) const { return wset && wset[f] >= 0 ? ds.weight_sum[(size_t)wset[f]] : ds.n_rows; }
    size_t put(const void *src, size_t bytes) {
        const size_t o = meta.size();
        meta.resize(o + ((bytes + 15) & ~size_t(15)));
        if (bytes) std::memcpy(meta.data() + o, src, bytes);
        return o;
    }
};

// every table names at least `min_cols` known columns, none twice, and has at most 2^28 cells -> cells_of
static int tables_check(mibn_ctx *h, const mibn_ctx::Dataset &ds, const std::string &what, int min_cols, const char *too_few, int32_t n,
                        const int64_t *scope_off, const int32_t *scope_cols, TableBatch &B) {
    B.cells_of.assign((size_t)n, 0);
    std::vector<int32_t> seen((size_t)ds.n_cols, -1);
    for (int f = 0; f < n; ++f) {
        const int64_t a = scope_off[f], b = scope_off[f + 1];
        if (b - a < min_cols) { h->err = what + " " + std::to_string(f) + " " + too_few; return MIBN_E_ARG; }
        int64_t cells = 1;
        for (int64_t k = a; k < b; ++k) {
            const int c = scope_cols[k];
            if (c < 0 || c >= ds.n_cols) { h->err = what + " " + std::to_string(f) + ": unknown column"; return MIBN_E_ARG; }
            if (seen[(size_t)c] == f) { h->err = what + " " + std::to_string(f) + " names a column twice"; return MIBN_E_ARG; }
            seen[(size_t)c] = f;
            cells *= ds.card[(size_t)c];
            if (cells > (int64_t(1) << 28)) { h->err = what + " " + std::to_string(f) + ": its table has more than " + std::to_string(int64_t(1) << 28) + " cells"; return MIBN_E_LIMIT; }
        }
        B.cells_of[(size_t)f] = cells;
    }
    for (int f = 0; B.wset && f < n; ++f)
        if (B.wset[f] < -1 || B.wset[f] >= ds.n_sets) { h->err = what + " " + std::to_string(f) + ": weight set " + std::to_string(B.wset[f]) + " outside [-1, " + std::to_string(ds.n_sets) + ")"; return MIBN_E_ARG; }
    return MIBN_OK;
}

// sub-batches: consecutive tables while they fit the cell budget (a larger table goes alone), each with its count_pack
static int tables_cut(mibn_ctx *h, const mibn_ctx::Dataset &ds, int32_t n, const int64_t *scope_off, const int32_t *scope_cols, TableBatch &B) {
    for (int f = 0; f < n;) {
        TableSub S;
        S.f0 = f;
        int64_t run = 0;
        while (f < n && (f == S.f0 || run + B.cells_of[(size_t)f] <= h->score_cells)) run += B.cells_of[(size_t)f++];
        S.f1 = f;
        S.cells = run;
        B.subs.push_back(std::move(S));
    }
    for (TableSub &S : B.subs) {
        S.off.assign((size_t)(S.f1 - S.f0) + 1, 0);
        for (int f = S.f0; f < S.f1; ++f) S.off[(size_t)(f - S.f0) + 1] = S.off[(size_t)(f - S.f0)] + B.cells_of[(size_t)f];
        const int rc = count_pack(ds.n_cols, ds.card.data(), S.f1 - S.f0, scope_off + S.f0, scope_cols, S.off.data(), S.pack, h->err);
        if (rc != MIBN_OK) return rc;
        if (B.wset) count_pack_weights(S.pack, S.f1 - S.f0, scope_off + S.f0, scope_cols, S.off.data(), B.wset + S.f0, h->weighted_share != 0, S.wpack);
        S.o_i64 = B.put(S.pack.i64.data(), S.pack.i64.size() * 8);
        S.o_i32 = B.put(S.pack.i32.data(), S.pack.i32.size() * 4);
        B.max_cells = std::max(B.max_cells, S.cells);
    }
    return MIBN_OK;
}

// the first device work of the call: buffers, events, the metadata upload
static int tables_begin(mibn_ctx *h, const TableBatch &B) {
    HIP_TRY(h, hipSetDevice(h->device));
    mibn_ctx::Score &X = h->sc;
    int rc;
    if ((rc = ensure(h, X.d_counts, (size_t)B.max_cells))) return rc;
    if ((rc = ensure(h, X.d_meta, B.meta.size() + 16))) return rc;
    while (X.ev.size() < 3 * B.subs.size()) {
        X.ev.emplace_back();
        HIP_TRY(h, X.ev.back().ensure());
    }
    const double t0 = now_ms();
    HIP_TRY(h, hipMemcpyAsync(X.d_meta, B.meta.data(), B.meta.size(), hipMemcpyHostToDevice, h->stream));
    h->stats.h2d_ms += now_ms() - t0;
    return MIBN_OK;
}

// the two phases of a sub-batch follow each other on the main stream, as do the sub-batches (they share the count buffer and the
// partials): no host synchronisation before the results are downloaded.  tables_count: events 3 s and 3 s + 1 around the counting;
// tables_reduced: event 3 s + 2 after the caller's kernels
static int tables_count(mibn_ctx *h, const mibn_ctx::Dataset &ds, TableBatch &B, size_t s) {
    mibn_ctx::Score &X = h->sc;
    TableSub &S = B.subs[s];
    HIP_TRY(h, hipMemsetAsync(X.d_counts, 0, 8 * (size_t)std::max<int64_t>(1, S.cells), h->stream));
    HIP_TRY(h, hipEventRecord(X.ev[3 * s], h->stream));
    const int32_t *d_i32 = reinterpret_cast<const int32_t *>(X.d_meta + S.o_i32);
    const int64_t *d_i64 = reinterpret_cast<const int64_t *>(X.d_meta + S.o_i64);
    if (B.wset) HIP_TRY(h, count_weighted_launch(h->stream, ds.d_codes, ds.n_rows, S.pack, S.wpack, d_i32, d_i64, ds.d_weights, X.d_counts));
    else HIP_TRY(h, count_launch(h->stream, ds.d_codes, ds.n_rows, S.pack, d_i32, d_i64, X.d_counts));
    S.count_launches = ds.n_rows > 0 ? (S.pack.n_big > 0) + (S.pack.n_small > 0) : 0;
    HIP_TRY(h, hipEventRecord(X.ev[3 * s + 1], h->stream));
    return MIBN_OK;
}

static int tables_reduced(mibn_ctx *h, size_t s) {
    HIP_TRY(h, hipGetLastError());
    HIP_TRY(h, hipEventRecord(h->sc.ev[3 * s + 2], h->stream));
    return MIBN_OK;
}

// after the stream is synchronised: last-call statistics, the counting under count_kernel (a weighted call: count_weighted_kernel,
// which also reads 4 bytes of weight per row and table) and the reduction under `slot`
static int tables_book(mibn_ctx *h, const mibn_ctx::Dataset &ds, const TableBatch &B, const int64_t *scope_off, int slot, double t_start) {
    mibn_ctx::Score &X = h->sc;
    mibn_kernel_stat &kc = h->kstats[B.wset ? kStatCountW : kStatCount], &ks = h->kstats[slot];
    for (size_t s = 0; s < B.subs.size(); ++s) {
        const TableSub &S = B.subs[s];
        float ms_c = 0, ms_s = 0;
        HIP_TRY(h, hipEventElapsedTime(&ms_c, X.ev[3 * s], X.ev[3 * s + 1]));
        HIP_TRY(h, hipEventElapsedTime(&ms_s, X.ev[3 * s + 1], X.ev[3 * s + 2]));
        const double n = (double)(S.f1 - S.f0);
        kc.launches += S.count_launches;
        kc.ms += ms_c;
        kc.alg_bytes += (double)ds.n_rows * (double)(scope_off[S.f1] - scope_off[S.f0]) + 8.0 * (double)S.cells;  // codes read per table member + the tables
        if (B.wset) kc.alg_bytes += 4.0 * (double)ds.n_rows * n;
        kc.items += n;
        ks.launches += S.reduce_launches;
        ks.ms += ms_s;
        ks.alg_bytes += S.reduce_bytes;
        ks.items += n;
        h->stats.kernel_ms += ms_c + ms_s;
        h->stats.n_launches += S.count_launches + S.reduce_launches;
    }
    h->stats.total_ms = now_ms() - t_start;
    return MIBN_OK;
}

// state and id checks of both entry points
static int tables_enter(mibn_ctx *h, int32_t id, const char *what) {
    if (int rc = check_state(h, kNeedDevice)) return rc;
    if (int rc = check_state(h, kNeedIdle)) return rc;
    if (id < 0 || (size_t)id >= h->datasets.size() || !h->datasets[(size_t)id].live) { h->err = std::string(what) + ": unknown or destroyed data set id"; return MIBN_E_ARG; }
    return MIBN_OK;
}

// mibn_score_families (wset = NULL) and mibn_score_families_w: one body.  The kernels take N as one launch argument, so the families of
// a sub-batch are reduced N by N - one class without weights and in a bootstrap, where every W_s = n_rows.
static int score_families_run(mibn_t *h, int32_t id, int32_t kind, double ess, int32_t n_fam, const int64_t *scope_off, const int32_t *scope_cols,
                              const int32_t *wset, double *scores) {
    int rc;
    if ((rc = tables_enter(h, id, "score"))) return rc;
    if (kind < MIBN_SCORE_LOGLIK || kind > MIBN_SCORE_K2) { h->err = "score: unknown kind"; return MIBN_E_ARG; }
    if (kind == MIBN_SCORE_BDEU && !(ess > 0 && ess < 1e300)) { h->err = "score: bdeu needs a finite equivalent sample size above 0"; return MIBN_E_ARG; }
    const mibn_ctx::Dataset &ds = h->datasets[(size_t)id];
    const double t_start = now_ms();
    reset_last_stats(h);
    if (n_fam == 0) return MIBN_OK;
    // ---- everything is checked and packed on the host before anything is launched
    TableBatch B;
    B.wset = wset;
    if ((rc = tables_check(h, ds, "score: family", 1, "is empty (the child comes last)", n_fam, scope_off, scope_cols, B))) return rc;
    if ((rc = tables_cut(h, ds, n_fam, scope_off, scope_cols, B))) return rc;
    struct Class {  // the families of one N
        int64_t n_rows = 0;
        std::vector<ScoreFam> small, big;
        std::vector<ScoreChunk> chunk;
        std::vector<ScoreBig> big_parts;
        size_t o_small = 0, o_big = 0, o_chunk = 0, o_bp = 0;  // in the metadata buffer
    };
    struct Sub {
        std::vector<Class> classes;  // in the order their N first occurs
        int32_t n_parts = 0;
    };
    std::vector<Sub> subs(B.subs.size());
    int32_t max_parts = 0;
    for (size_t s = 0; s < subs.size(); ++s) {
        const TableSub &T = B.subs[s];
        Sub &U = subs[s];
        for (int f = T.f0; f < T.f1; ++f) {
            const int64_t n_rows = B.rows_of(ds, f);
            size_t c = 0;
            while (c < U.classes.size() && U.classes[c].n_rows != n_rows) ++c;
            if (c == U.classes.size()) { U.classes.emplace_back(); U.classes[c].n_rows = n_rows; }
            Class &S = U.classes[c];
            ScoreFam F;
            F.off = T.off[(size_t)(f - T.f0)];
            F.r = ds.card[(size_t)scope_cols[scope_off[f + 1] - 1]];
            F.q = B.cells_of[(size_t)f] / F.r;
            F.out = f;
            if (F.q * F.r <= kScoreWaveCells) {
                S.small.push_back(F);
            } else {
                const int64_t per = score_chunk_configs(F.r);
                ScoreBig G;
                G.part0 = U.n_parts;
                G.n_parts = (int32_t)((F.q + per - 1) / per);
                for (int32_t i = 0; i < G.n_parts; ++i) S.chunk.push_back(ScoreChunk{(int32_t)S.big.size(), U.n_parts + i, (int64_t)i * per});
                U.n_parts += G.n_parts;
                S.big.push_back(F);
                S.big_parts.push_back(G);
            }
        }
        max_parts = std::max(max_parts, U.n_parts);
        for (Class &S : U.classes) {
            S.o_small = B.put(S.small.data(), S.small.size() * sizeof(ScoreFam));
            S.o_big = B.put(S.big.data(), S.big.size() * sizeof(ScoreFam));
            S.o_chunk = B.put(S.chunk.data(), S.chunk.size() * sizeof(ScoreChunk));
            S.o_bp = B.put(S.big_parts.data(), S.big_parts.size() * sizeof(ScoreBig));
        }
    }
    // ---- device
    if ((rc = tables_begin(h, B))) return rc;
    mibn_ctx::Score &X = h->sc;
    if ((rc = ensure(h, X.d_f64, (size_t)n_fam + (size_t)max_parts + 2))) return rc;
    const hipStream_t S0 = h->stream;
    double *d_scores = X.d_f64, *d_parts = X.d_f64 + n_fam;
    for (size_t s = 0; s < subs.size(); ++s) {
        if ((rc = tables_count(h, ds, B, s))) return rc;
        TableSub &T = B.subs[s];
        for (const Class &S : subs[s].classes) {
            ScoreArgs A;
            A.counts = X.d_counts;
            A.small = reinterpret_cast<const ScoreFam *>(X.d_meta + S.o_small);
            A.big = reinterpret_cast<const ScoreFam *>(X.d_meta + S.o_big);
            A.chunk = reinterpret_cast<const ScoreChunk *>(X.d_meta + S.o_chunk);
            A.big_parts = reinterpret_cast<const ScoreBig *>(X.d_meta + S.o_bp);
            A.parts = d_parts;
            A.scores = d_scores;
            A.ess = ess;
            A.n_rows = S.n_rows;
            A.kind = kind;
            A.n_small = (int32_t)S.small.size();
            A.n_big = (int32_t)S.big.size();
            constexpr int kPerWG = kScoreWG / 64;
            if (A.n_small) {
                hipLaunchKernelGGL(score_kernel, dim3((unsigned)((A.n_small + kPerWG - 1) / kPerWG)), dim3(kScoreWG), 0, S0, A);
                T.reduce_launches += 1;
            }
            if (A.n_big) {
                hipLaunchKernelGGL(score_chunk_kernel, dim3((unsigned)S.chunk.size()), dim3(kScoreWG), 0, S0, A);
                hipLaunchKernelGGL(score_finish_kernel, dim3((unsigned)((A.n_big + kPerWG - 1) / kPerWG)), dim3(kScoreWG), 0, S0, A);
                T.reduce_launches += 2;
            }
        }
        T.reduce_bytes = 8.0 * ((double)T.cells + (double)(T.f1 - T.f0) + 2.0 * (double)subs[s].n_parts);
        if ((rc = tables_reduced(h, s))) return rc;
    }
    const double t0 = now_ms();
    HIP_TRY(h, hipMemcpyAsync(scores, d_scores, (size_t)n_fam * 8, hipMemcpyDeviceToHost, S0));
    HIP_TRY(h, hipStreamSynchronize(S0));
    h->stats.d2h_ms += now_ms() - t0;
    return tables_book(h, ds, B, scope_off, kStatScore, t_start);
}

extern "C" int mibn_score_families(mibn_t *h, int32_t id, int32_t kind, double ess, int32_t n_fam, const int64_t *scope_off, const int32_t *scope_cols,
                                   double *scores) {
    if (!h || n_fam < 0 || !scope_off || (n_fam && (!scope_cols || !scores))) return MIBN_E_ARG;
    return score_families_run(h, id, kind, ess, n_fam, scope_off, scope_cols, nullptr, scores);
}

extern "C" int mibn_score_families_w(mibn_t *h, int32_t id, int32_t kind, double ess, int32_t n_fam, const int64_t *scope_off, const int32_t *scope_cols,
                                     const int32_t *wset, double *scores) {
    if (!h || n_fam < 0 || !scope_off || (n_fam && (!scope_cols || !scores || !wset))) return MIBN_E_ARG;
    static const int32_t none = -1;  // (n_fam = 0: still the weighted path)
    return score_families_run(h, id, kind, ess, n_fam, scope_off, scope_cols, wset ? wset : &none, scores);
}

// mibn_ci_tests (wset = NULL) and mibn_ci_tests_w: one body (the kernels read no N)
static int ci_tests_run(mibn_t *h, int32_t id, int32_t kind, int32_t n_tests, const int64_t *scope_off, const int32_t *scope_cols, const int32_t *wset,
                        double *stat, int64_t *adj_dof) {
    int rc;
    if ((rc = tables_enter(h, id, "ci"))) return rc;
    if (kind != MIBN_CI_G2 && kind != MIBN_CI_X2) { h->err = "ci: unknown kind"; return MIBN_E_ARG; }
    const mibn_ctx::Dataset &ds = h->datasets[(size_t)id];
    if (ds.n_rows >= (int64_t(1) << 31)) { h->err = "ci: the data set has 2^31 rows or more (the statistics' products are 64-bit integers)"; return MIBN_E_LIMIT; }
    for (int f = 0; wset && f < n_tests; ++f)
        if (wset[f] >= 0 && wset[f] < ds.n_sets && ds.weight_sum[(size_t)wset[f]] >= (int64_t(1) << 31)) { h->err = "ci: test " + std::to_string(f) + ": its weight set sums to 2^31 or more (the statistics' products are 64-bit integers)"; return MIBN_E_LIMIT; }
    const double t_start = now_ms();
    reset_last_stats(h);
    if (n_tests == 0) return MIBN_OK;
    // ---- everything is checked and packed on the host before anything is launched
    TableBatch B;
    B.wset = wset;
    if ((rc = tables_check(h, ds, "ci: test", 2, "names fewer than two columns (conditioning columns, then X, then Y)", n_tests, scope_off, scope_cols, B))) return rc;
    if ((rc = tables_cut(h, ds, n_tests, scope_off, scope_cols, B))) return rc;
    struct Sub {
        std::vector<CiItem> lane, wave;  // lane: by group size, 64 first
        std::vector<CiBig> big;
        int32_t lane0[kCiClasses + 1] = {}, item0[kCiClasses + 1] = {};
        int32_t n_parts = 0;
        size_t o_lane = 0, o_wave = 0, o_big = 0;
    };
    std::vector<Sub> subs(B.subs.size());
    int32_t max_parts = 0;
    for (size_t s = 0; s < subs.size(); ++s) {
        const TableSub &T = B.subs[s];
        Sub &S = subs[s];
        std::vector<CiItem> by_class[kCiClasses];
        auto add = [&](const CiItem &I, int64_t strata_of_table) {
            if (I.rx * I.ry > kCiLaneCells) return S.wave.push_back(I);
            int k = 0;  // group of 64 >> k lanes
            for (const int32_t g = ci_group(strata_of_table); (64 >> k) > g;) ++k;
            by_class[k].push_back(I);
        };
        for (int f = T.f0; f < T.f1; ++f) {
            CiItem I;
            I.off = T.off[(size_t)(f - T.f0)];
            I.rx = ds.card[(size_t)scope_cols[scope_off[f + 1] - 2]];
            I.ry = ds.card[(size_t)scope_cols[scope_off[f + 1] - 1]];
            const int64_t cells = B.cells_of[(size_t)f], sz = (int64_t)I.rx * I.ry, q = cells / sz;
            if (cells <= kCiWaveCells) {
                I.nz = (int32_t)q;
                I.out = f;
                add(I, q);
                continue;
            }
            const int64_t per = ci_chunk_strata(sz);
            CiBig G;
            G.part0 = n_tests + S.n_parts;
            G.n_parts = (int32_t)((q + per - 1) / per);
            G.out = f;
            for (int32_t c = 0; c < G.n_parts; ++c) {
                CiItem P = I;
                P.off = I.off + (int64_t)c * per * sz;
                P.nz = (int32_t)std::min<int64_t>(per, q - (int64_t)c * per);
                P.out = G.part0 + c;
                add(P, 64);  // (a chunk of the lane form: always a whole wave)
            }
            S.n_parts += G.n_parts;
            S.big.push_back(G);
        }
        int64_t lanes = 0;
        for (int k = 0; k < kCiClasses; ++k) {
            S.lane0[k] = (int32_t)lanes;
            S.item0[k] = (int32_t)S.lane.size();
            lanes += (int64_t)by_class[k].size() * (64 >> k);
            S.lane.insert(S.lane.end(), by_class[k].begin(), by_class[k].end());
        }
        if (lanes >= (int64_t(1) << 31)) { h->err = "ci: a sub-batch needs 2^31 lanes or more (lower the option score_cells)"; return MIBN_E_LIMIT; }
        S.lane0[kCiClasses] = (int32_t)lanes;
        S.item0[kCiClasses] = (int32_t)S.lane.size();
        max_parts = std::max(max_parts, S.n_parts);
        S.o_lane = B.put(S.lane.data(), S.lane.size() * sizeof(CiItem));
        S.o_wave = B.put(S.wave.data(), S.wave.size() * sizeof(CiItem));
        S.o_big = B.put(S.big.data(), S.big.size() * sizeof(CiBig));
    }
    // ---- device
    if ((rc = tables_begin(h, B))) return rc;
    mibn_ctx::Score &X = h->sc;
    if ((rc = ensure(h, X.d_f64, (size_t)n_tests + (size_t)max_parts + 2))) return rc;
    if ((rc = ensure(h, X.d_i64, (size_t)n_tests + (size_t)max_parts + 2))) return rc;
    const hipStream_t S0 = h->stream;
    for (size_t s = 0; s < subs.size(); ++s) {
        const Sub &S = subs[s];
        if ((rc = tables_count(h, ds, B, s))) return rc;
        CiArgs A;
        A.counts = X.d_counts;
        A.lane_items = reinterpret_cast<const CiItem *>(X.d_meta + S.o_lane);
        A.wave_items = reinterpret_cast<const CiItem *>(X.d_meta + S.o_wave);
        A.big = reinterpret_cast<const CiBig *>(X.d_meta + S.o_big);
        A.stat = X.d_f64;
        A.dof = X.d_i64;
        A.kind = kind;
        A.n_wave = (int32_t)S.wave.size();
        A.n_big = (int32_t)S.big.size();
        std::copy(S.lane0, S.lane0 + kCiClasses + 1, A.lane0);
        std::copy(S.item0, S.item0 + kCiClasses + 1, A.item0);
        TableSub &T = B.subs[s];
        if (!S.lane.empty()) {
            hipLaunchKernelGGL(ci_lane_kernel, dim3((unsigned)((S.lane0[kCiClasses] + kCiWG - 1) / kCiWG)), dim3(kCiWG), 0, S0, A);
            T.reduce_launches += 1;
        }
        if (A.n_wave) {
            hipLaunchKernelGGL(ci_wave_kernel, dim3((unsigned)A.n_wave), dim3(64), 0, S0, A);
            T.reduce_launches += 1;
        }
        if (A.n_big) {
            constexpr int kPerWG = kCiWG / 64;
            hipLaunchKernelGGL(ci_finish_kernel, dim3((unsigned)((A.n_big + kPerWG - 1) / kPerWG)), dim3(kCiWG), 0, S0, A);
            T.reduce_launches += 1;
        }
        T.reduce_bytes = 8.0 * (double)T.cells + 16.0 * ((double)(T.f1 - T.f0) + 2.0 * (double)S.n_parts);
        if ((rc = tables_reduced(h, s))) return rc;
    }
    const double t0 = now_ms();
    HIP_TRY(h, hipMemcpyAsync(stat, X.d_f64, (size_t)n_tests * 8, hipMemcpyDeviceToHost, S0));
    HIP_TRY(h, hipMemcpyAsync(adj_dof, X.d_i64, (size_t)n_tests * 8, hipMemcpyDeviceToHost, S0));
    HIP_TRY(h, hipStreamSynchronize(S0));
    h->stats.d2h_ms += now_ms() - t0;
    return tables_book(h, ds, B, scope_off, kStatCiTest, t_start);
}

extern "C" int mibn_ci_tests(mibn_t *h, int32_t id, int32_t kind, int32_t n_tests, const int64_t *scope_off, const int32_t *scope_cols, double *stat,
                             int64_t *adj_dof) {
    if (!h || n_tests < 0 || !scope_off || (n_tests && (!scope_cols || !stat || !adj_dof))) return MIBN_E_ARG;
    return ci_tests_run(h, id, kind, n_tests, scope_off, scope_cols, nullptr, stat, adj_dof);
}

extern "C" int mibn_ci_tests_w(mibn_t *h, int32_t id, int32_t kind, int32_t n_tests, const int64_t *scope_off, const int32_t *scope_cols,
                               const int32_t *wset, double *stat, int64_t *adj_dof) {
    if (!h || n_tests < 0 || !scope_off || (n_tests && (!scope_cols || !stat || !adj_dof || !wset))) return MIBN_E_ARG;
    static const int32_t none = -1;
    return ci_tests_run(h, id, kind, n_tests, scope_off, scope_cols, wset ? wset : &none, stat, adj_dof);
}

// ---- mibn_best_dag and mibn_arc_posteriors: one driver frame.  Both check and plan (dag_plan.h), make room for their tables,
// upload the candidates, run fill + scatter + the passes and then their levels on the main stream with an event between phases,
// download, synchronise once and turn the events into statistics rows.  DagFrame holds what the calls share, the
// two *_run functions what differs.  Tables above kDagKeepBytes are freed when the call returns (2.6 GB at n = 24 would otherwise
// stay with a context that may never ask again).
constexpr size_t kDagKeepBytes = size_t(1) << 28;

template <class T>
static hipError_t dag_room(DevBuf<T> &buf, size_t need) {  // exactly `need`: no headroom on gigabytes
    if (need <= buf.cap()) return hipSuccess;
    const hipError_t e = buf.reset(need);
    if (e != hipSuccess) (void)hipGetLastError();  // (a refused allocation must not be what a later call's launch check finds)
    return e;
}

struct DagRow {  // a statistics row: its slot, launches, algorithmic bytes and items; row k runs between the events k and k + 1
    int slot;
    double launches, bytes, items;
    void add(double b) { launches += 1; bytes += b; }
};

struct DagFrame {
    mibn_t *h;
    mibn_ctx::Dag &X;
    int32_t n = 0;
    int64_t n_fam = 0;
    DagPlan D;
    size_t bps = 0, subsets = 0, fam = 0;  // entries of all children's tables, subsets, max(1, n_fam)
    hipStream_t S0 = nullptr;
    dim3 wg{kDagWG}, per_fam;
    double t_start = 0, t_mark = 0;
    int marks = 0;  // events recorded
    // the block d_io, carved in descending alignment: the candidates, then what the call asks for
    double *d_fam = nullptr;
    int32_t *d_child = nullptr;
    uint32_t *d_par = nullptr;
    char *d_free = nullptr;
    template <class T>
    T *carve(size_t count) { return reinterpret_cast<T *>(std::exchange(d_free, d_free + sizeof(T) * count)); }

    // the entry checks and the plan
    int enter(const char *who, int32_t n_vars, int64_t n_fam_, const int32_t *fam_child, const uint32_t *fam_parents, const double *fam_score) {
        if (int rc = check_state(h, kNeedDevice)) return rc;
        if (int rc = check_state(h, kNeedIdle)) return rc;
        t_start = now_ms();
        reset_last_stats(h);
        static_assert(MIBN_ARC_POSTERIOR_MAX_VARS == MIBN_BEST_DAG_MAX_VARS, "dag_check's limit is the one of both calls");
        if (int rc = dag_check(who, n_vars, n_fam_, fam_child, fam_parents, fam_score, h->err)) return rc;
        n = n_vars, n_fam = n_fam_, S0 = h->stream;
        D = dag_plan(n, h->dag_tile_bits, h->dag_group_bits);
        HIP_TRY(h, hipSetDevice(h->device));
        bps = (size_t)n * (size_t)D.entries, subsets = size_t(1) << n, fam = (size_t)std::max<int64_t>(1, n_fam);
        per_fam = dim3((unsigned)((fam + kDagWG - 1) / kDagWG));
        return MIBN_OK;
    }
    // d_io <- [fam_score | fam_child | fam_parents] (16 fam bytes: what follows stays 16-aligned), then `rest` bytes for the call
    // to carve; the events
    int upload(const int32_t *fam_child, const uint32_t *fam_parents, const double *fam_score, size_t rest) {
        HIP_TRY(h, X.d_io.ensure(16 * fam + rest));
        for (Event &e : X.ev) HIP_TRY(h, e.ensure());
        d_free = X.d_io;
        d_fam = carve<double>(fam), d_child = carve<int32_t>(fam), d_par = carve<uint32_t>(fam);
        const double t0 = now_ms();
        if (n_fam) {
            HIP_TRY(h, hipMemcpyAsync(d_fam, fam_score, 8 * (size_t)n_fam, hipMemcpyHostToDevice, S0));
            HIP_TRY(h, hipMemcpyAsync(d_child, fam_child, 4 * (size_t)n_fam, hipMemcpyHostToDevice, S0));
            HIP_TRY(h, hipMemcpyAsync(d_par, fam_parents, 4 * (size_t)n_fam, hipMemcpyHostToDevice, S0));
        }
        h->stats.h2d_ms += now_ms() - t0;
        return MIBN_OK;
    }
    // the end of a phase: its launches are checked and the next event is recorded
    int mark() {
        if (marks) HIP_TRY(h, hipGetLastError());
        HIP_TRY(h, hipEventRecord(X.ev[marks++], S0));
        t_mark = now_ms();
        return MIBN_OK;
    }
    // the first phase of both calls, launches and bytes counted: fill(grid), scatter() if there are candidates, pass(grid, P) for
    // each pass of the plan.  A table entry has `entry_bytes` (written by fill, read and written by a pass), a candidate moves `fam_bytes`.
    template <class Fill, class Scatter, class Pass>
    DagRow fill_scatter_passes(int slot, double entry_bytes, double fam_bytes, Fill &&fill, Scatter &&scatter, Pass &&pass) const {
        DagRow row{slot, 0, 0, (double)n_fam};
        fill(dim3((unsigned)std::min<size_t>((bps + kDagWG - 1) / kDagWG, 65536)));
        row.add(entry_bytes * (double)bps);
        if (n_fam) {
            scatter();
            row.add(fam_bytes * (double)n_fam);
        }
        for (const DagPass &P : D.passes) {
            pass(dim3((unsigned)D.grid(P)), P);
            row.add(2.0 * entry_bytes * (double)bps);
        }
        return row;
    }
    // after the downloads were queued: the one synchronisation, then the events as statistics rows
    int finish(std::initializer_list<DagRow> rows) {
        HIP_TRY(h, hipStreamSynchronize(S0));
        h->stats.d2h_ms += now_ms() - t_mark;
        for (size_t k = 0; k < rows.size(); ++k) {
            const DagRow &r = rows.begin()[k];
            float ms = 0;
            HIP_TRY(h, hipEventElapsedTime(&ms, X.ev[k], X.ev[k + 1]));
            book_stat(h, r.slot, r.launches, ms, r.bytes, r.items, true, false);
            h->stats.kernel_ms += ms, h->stats.n_launches += r.launches, h->stats.alg_bytes += r.bytes;
        }
        h->stats.total_ms = now_ms() - t_start;
        return MIBN_OK;
    }
};

// mibn_best_dag: fill + scatter + the passes of phase A | the n + 1 levels of phase B and the traceback: two statistics rows
static int best_dag_run(mibn_t *h, int32_t n, int64_t n_fam, const int32_t *fam_child, const uint32_t *fam_parents, const double *fam_score,
                        uint32_t *parents_out, int32_t *order_out, double *total_out) {
    DagFrame F{h, h->dag};
    if (int rc = F.enter("best_dag", n, n_fam, fam_child, fam_parents, fam_score)) return rc;
    mibn_ctx::Dag &X = F.X;
    const size_t bps = F.bps, subsets = F.subsets;
    struct Release {  // the call's tables, on every exit (hipFree waits for the device)
        mibn_ctx::Dag &X;
        bool on;
        ~Release() { if (on) (void)X.d_score.release(), (void)X.d_mask.release(), (void)X.d_best.release(), (void)X.d_sink.release(); }
    } release{X, 12 * bps + 9 * subsets > kDagKeepBytes};
    HIP_TRY(h, dag_room(X.d_score, bps));
    HIP_TRY(h, dag_room(X.d_mask, bps));
    HIP_TRY(h, dag_room(X.d_best, subsets));
    HIP_TRY(h, dag_room(X.d_sink, subsets));
    if (int rc = F.upload(fam_child, fam_parents, fam_score, 8 + 8 * (size_t)n)) return rc;
    double *d_total = F.carve<double>(1);
    uint32_t *d_pout = F.carve<uint32_t>((size_t)n);
    int32_t *d_order = F.carve<int32_t>((size_t)n);
    const hipStream_t S0 = F.S0;
    // phase A
    if (int rc = F.mark()) return rc;
    const DagRow a = F.fill_scatter_passes(
        kStatDagSubset, 12.0, 28.0, [&](dim3 grid) { hipLaunchKernelGGL(dag_fill_kernel, grid, F.wg, 0, S0, X.d_score.get(), X.d_mask.get(), (int64_t)bps); },
        [&] { hipLaunchKernelGGL(dag_scatter_kernel, F.per_fam, F.wg, 0, S0, F.d_child, F.d_par, F.d_fam, n_fam, n, X.d_score.get(), X.d_mask.get()); },
        [&](dim3 grid, const DagPass &P) { hipLaunchKernelGGL(dag_subset_kernel, grid, F.wg, 0, S0, X.d_score.get(), X.d_mask.get(), P, n, F.D.tiles_per_child(P)); });
    if (int rc = F.mark()) return rc;
    // phase B and the traceback
    for (int32_t level = 0; level <= n; ++level)
        hipLaunchKernelGGL(dag_sink_kernel, dim3((unsigned)((subsets + kDagWG - 1) / kDagWG)), F.wg, 0, S0, X.d_score.get(), X.d_best.get(), X.d_sink.get(), n, level);
    hipLaunchKernelGGL(dag_traceback_kernel, dim3(1), dim3(64), 0, S0, X.d_mask.get(), X.d_best.get(), X.d_sink.get(), n, d_pout, d_order, d_total);
    if (int rc = F.mark()) return rc;
    HIP_TRY(h, hipMemcpyAsync(total_out, d_total, 8, hipMemcpyDeviceToHost, S0));
    HIP_TRY(h, hipMemcpyAsync(parents_out, d_pout, 4 * (size_t)n, hipMemcpyDeviceToHost, S0));
    HIP_TRY(h, hipMemcpyAsync(order_out, d_order, 4 * (size_t)n, hipMemcpyDeviceToHost, S0));
    // phase B: every bps score and every best entry read once per member, best and sink written once per subset; the traceback's 2 n reads
    return F.finish({a, {kStatDagSink, (double)n + 2.0, 16.0 * (double)bps + 9.0 * (double)subsets, (double)subsets}});
}

extern "C" int mibn_best_dag(mibn_t *h, int32_t n_vars, int64_t n_fam, const int32_t *fam_child, const uint32_t *fam_parents, const double *fam_score,
                             uint32_t *parents_out, int32_t *order_out, double *total_out) {
    if (!h || n_fam < 0 || (n_fam && (!fam_child || !fam_parents || !fam_score)) || !parents_out || !order_out || !total_out) return MIBN_E_ARG;
    return drained_on_error(h, best_dag_run(h, n_vars, n_fam, fam_child, fam_parents, fam_score, parents_out, order_out, total_out), drain_main_unchecked);
}

// mibn_arc_posteriors: fill + scatter + the passes of the subset sum | the n + 1 levels of L and R | the passes of the superset sum
// (the first forms g from L and R) | the candidate kernel and the arc sums: four statistics rows
static int arc_posteriors_run(mibn_t *h, int32_t n, int64_t n_fam, const int32_t *fam_child, const uint32_t *fam_parents, const double *fam_score,
                              double *log_post_out, double *arc_out, double *log_evidence_out) {
    DagFrame F{h, h->dag};
    if (int rc = F.enter("arc_posteriors", n, n_fam, fam_child, fam_parents, fam_score)) return rc;
    std::vector<DagPass> down = F.D.passes;  // the superset sum: the same passes; n = 1 has none, and g is formed by a pass without bits
    if (down.empty()) down.push_back(DagPass{0, 0, 0});
    std::vector<double> centre((size_t)n);
    dag_centres(n, n_fam, fam_child, fam_score, centre.data());
    mibn_ctx::Dag &X = F.X;
    const size_t bps = F.bps, subsets = F.subsets, nn = (size_t)n * (size_t)n;
    const int64_t segments = dag_arc_segments(n_fam);
    struct Release {  // the call's tables, on every exit (hipFree waits for the device)
        mibn_ctx::Dag &X;
        bool on;
        ~Release() { if (on) (void)X.d_score.release(), (void)X.d_best.release(), (void)X.d_right.release(); }
    } release{X, 8 * bps + 16 * subsets > kDagKeepBytes};
    HIP_TRY(h, dag_room(X.d_score, bps));
    HIP_TRY(h, dag_room(X.d_best, subsets));
    HIP_TRY(h, dag_room(X.d_right, subsets));
    static const std::vector<uint32_t> binom = dag_binomials();
    if (int rc = F.upload(fam_child, fam_parents, fam_score, 8 * ((size_t)n + F.fam + nn + nn * (size_t)segments) + 4 * binom.size())) return rc;
    double *d_centre = F.carve<double>((size_t)n), *d_post = F.carve<double>(F.fam), *d_arc = F.carve<double>(nn), *d_part = F.carve<double>(nn * (size_t)segments);
    uint32_t *d_binom = F.carve<uint32_t>(binom.size());
    const hipStream_t S0 = F.S0;
    const double t0 = now_ms();
    HIP_TRY(h, hipMemcpyAsync(d_centre, centre.data(), 8 * (size_t)n, hipMemcpyHostToDevice, S0));  // (pageable: staged before the call returns)
    HIP_TRY(h, hipMemcpyAsync(d_binom, binom.data(), 4 * binom.size(), hipMemcpyHostToDevice, S0));
    h->stats.h2d_ms += now_ms() - t0;
    double *alpha = X.d_score.get(), *L = X.d_best.get(), *R = X.d_right.get();
    // the subset sum
    if (int rc = F.mark()) return rc;
    const DagRow a = F.fill_scatter_passes(
        kStatDagPostSubset, 8.0, 32.0, [&](dim3 grid) { hipLaunchKernelGGL(dag_post_fill_kernel, grid, F.wg, 0, S0, alpha, (int64_t)bps); },
        [&] { hipLaunchKernelGGL(dag_post_scatter_kernel, F.per_fam, F.wg, 0, S0, F.d_child, F.d_par, F.d_fam, d_centre, n_fam, n, alpha); },
        [&](dim3 grid, const DagPass &P) { hipLaunchKernelGGL(dag_post_subset_kernel, grid, F.wg, 0, S0, alpha, P, n, F.D.tiles_per_child(P)); });
    if (int rc = F.mark()) return rc;
    // L and R
    for (int32_t level = 0; level <= n; ++level)
        hipLaunchKernelGGL(dag_post_level_kernel, dim3((binom[(size_t)n * kDagBinomStride + (size_t)level] + kDagWG - 1) / kDagWG), F.wg, 0, S0, alpha, L, R, d_binom,
                           n, level);
    if (int rc = F.mark()) return rc;
    // the superset sum of g into alpha's storage
    DagRow c{kStatDagPostSuperset, 0, 0, (double)bps};
    for (size_t k = 0; k < down.size(); ++k) {
        hipLaunchKernelGGL(dag_post_superset_kernel, dim3((unsigned)F.D.grid(down[k])), F.wg, 0, S0, alpha, L, R, down[k], n, F.D.tiles_per_child(down[k]), (int32_t)(k == 0));
        c.add((k == 0 ? 24.0 : 16.0) * (double)bps);  // the first pass reads L and R per entry and writes the entry
    }
    if (int rc = F.mark()) return rc;
    // the candidates' posteriors and the arc sums
    double launches_d = 2;
    if (n_fam) {
        hipLaunchKernelGGL(dag_post_candidate_kernel, F.per_fam, F.wg, 0, S0, F.d_child, F.d_par, F.d_fam, d_centre, alpha, L, n_fam, n, d_post);
        launches_d += 1;
    }
    hipLaunchKernelGGL(dag_post_arc_kernel, dim3((unsigned)segments, (unsigned)n), F.wg, 0, S0, F.d_child, F.d_par, d_post, n_fam, n, d_part);
    hipLaunchKernelGGL(dag_post_arc_sum_kernel, dim3((unsigned)((nn + kDagWG - 1) / kDagWG)), F.wg, 0, S0, d_part, segments, n, d_arc);
    if (int rc = F.mark()) return rc;
    double l_full = 0;
    HIP_TRY(h, hipMemcpyAsync(&l_full, L + (subsets - 1), 8, hipMemcpyDeviceToHost, S0));
    HIP_TRY(h, hipMemcpyAsync(arc_out, d_arc, 8 * nn, hipMemcpyDeviceToHost, S0));
    if (n_fam) HIP_TRY(h, hipMemcpyAsync(log_post_out, d_post, 8 * (size_t)n_fam, hipMemcpyDeviceToHost, S0));
    // L and R: every alpha entry read twice and every L / R entry once per member, both written once per subset
    const double bytes_b = 32.0 * (double)bps + 16.0 * (double)subsets;
    // a candidate's 24 bytes, its Gamma and its log_post; the arc kernel reads child per (candidate, child), masks and log_post once
    const double bytes_d = 40.0 * (double)n_fam + (4.0 * (double)n + 12.0) * (double)n_fam + 8.0 * (double)nn * ((double)segments + 1.0);
    if (int rc = F.finish({a, {kStatDagPostLevel, (double)n + 1.0, bytes_b, (double)subsets}, c, {kStatDagPostArc, launches_d, bytes_d, (double)n_fam}})) return rc;
    *log_evidence_out = dag_log_evidence(l_full, n, centre.data());
    return MIBN_OK;
}

extern "C" int mibn_arc_posteriors(mibn_t *h, int32_t n_vars, int64_t n_fam, const int32_t *fam_child, const uint32_t *fam_parents, const double *fam_score,
                                   double *log_post_out, double *arc_out, double *log_evidence_out) {
    if (!h || n_fam < 0 || (n_fam && (!fam_child || !fam_parents || !fam_score || !log_post_out)) || !arc_out || !log_evidence_out) return MIBN_E_ARG;
    return drained_on_error(h, arc_posteriors_run(h, n_vars, n_fam, fam_child, fam_parents, fam_score, log_post_out, arc_out, log_evidence_out),
                            drain_main_unchecked);
}

extern "C" int mibn_plan_order(mibn_t *h, int32_t n_q, const int32_t *q_vars, int32_t n_e, const int32_t *e_vars,
                               int32_t *order, int32_t *n) {
    if (!h || !order || !n) return MIBN_E_ARG;
    if (int rc = check_state(h, kNeedNet)) return rc;
    Request rq;
    rq.nq = n_q; rq.qvars = q_vars; rq.ne = n_e; rq.evars = e_vars;
    std::string e = validate_request(h->net, rq);
    if (!e.empty()) { h->err = e; return MIBN_E_ARG; }
    std::vector<uint32_t> prog;
    std::vector<int32_t> ord;
    PlanStats st;
    st.order = &ord;
    e = plan_request(h->net, rq, prog, st);
    if (!e.empty()) { h->err = e; return MIBN_E_LIMIT; }
    *n = (int32_t)ord.size();
    std::copy(ord.begin(), ord.end(), order);
    return MIBN_OK;
}

extern "C" int mibn_estimate_costs(mibn_t *h, int64_t B, const int64_t *q_off, const int32_t *q_vars, const int64_t *e_off,
                                   const int32_t *e_vars, double *cost) {
    if (!h || B < 0 || !q_off || !e_off || (B && (!q_vars || !cost))) return MIBN_E_ARG;
    if (int rc = check_state(h, kNeedNet)) return rc;
    ensure_pool(h);
    estimate_costs(h->net, *h->pool, B, q_off, q_vars, e_off, e_vars, cost);
    return MIBN_OK;
}

extern "C" int mibn_device_synchronize(mibn_t *h) {
    if (!h) return MIBN_E_ARG;
    if (h->planner_only) return MIBN_OK;
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, hipDeviceSynchronize());
    return MIBN_OK;
}

// ---------------------------------------------------------------------------------------------------- RCCL
// One process per GPU; the data path has no collective (independent request / chain shards), these are the final
// gather / reduce over xGMI.  librccl.so (573 MB) is loaded on the first mibn_comm_* call only.
namespace {

int comm_load(mibn_ctx *h) {
    mibn_ctx::Comm &c = h->comm;
    if (c.dl) return MIBN_OK;
    const char *env = std::getenv("MIBN_RCCL_LIB");
    const char *cands[] = {env, "librccl.so.1", "/opt/rocm/lib/librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so"};
    for (const char *name : cands) {
        if (!name || !*name) continue;
        if ((c.dl = dlopen(name, RTLD_NOW | RTLD_LOCAL))) break;
    }
    if (!c.dl) { h->err = std::string("cannot load librccl.so: ") + dlerror(); return MIBN_E_COMM; }
#define MIBN_SYM(field, sym)                                                                  \
    c.field = reinterpret_cast<decltype(c.field)>(dlsym(c.dl, #sym));                         \
    if (!c.field) { h->err = "librccl.so lacks " #sym; dlclose(c.dl); c.dl = nullptr; return MIBN_E_COMM; }
    MIBN_SYM(GetUniqueId, ncclGetUniqueId)
    MIBN_SYM(CommInitRank, ncclCommInitRank)
    MIBN_SYM(CommDestroy, ncclCommDestroy)
    MIBN_SYM(CommCount, ncclCommCount)
    MIBN_SYM(CommUserRank, ncclCommUserRank)
    MIBN_SYM(AllGather, ncclAllGather)
    MIBN_SYM(Reduce, ncclReduce)
    MIBN_SYM(AllReduce, ncclAllReduce)
    MIBN_SYM(GetErrorString, ncclGetErrorString)
#undef MIBN_SYM
    return MIBN_OK;
}

#define NCCL_TRY(h, expr)                                                                             \
    do {                                                                                              \
        ncclResult_t r_ = (expr);                                                                     \
        if (r_ != ncclSuccess) {                                                                      \
            (h)->err = std::string(#expr) + ": " + (h)->comm.GetErrorString(r_);                      \
            return MIBN_E_COMM;                                                                       \
        }                                                                                             \
    } while (0)

int comm_ready(mibn_ctx *h) {
    if (!h) return MIBN_E_ARG;
    if (h->planner_only) { h->err = "planner-only context: no HIP device bound"; return MIBN_E_NODEVICE; }
    if (!h->comm.comm) { h->err = "mibn_comm_init first"; return MIBN_E_STATE; }
    HIP_TRY(h, hipSetDevice(h->device));
    return MIBN_OK;
}

int comm_buf(mibn_ctx *h, DevBuf<char> &buf, size_t bytes) {
    if (bytes > buf.cap()) HIP_TRY(h, buf.reset(bytes + bytes / 4 + 256));
    return MIBN_OK;
}

}  // namespace

// dlopen + symbol resolution only: what can fail on ONE rank of a node, checked before anybody enters the collective init.
// (ncclGetUniqueId is for rank 0 alone: on any other rank it starts a bootstrap listener thread and a socket that wait for
// `world` connections which never arrive - ADVICE r3.)
extern "C" int mibn_comm_probe(mibn_t *h) {
    if (!h) return MIBN_E_ARG;
    if (h->planner_only) { h->err = "planner-only context: no HIP device bound"; return MIBN_E_NODEVICE; }
    return comm_load(h);
}

// One line about this context's device for the launch log: name, PCI bus id, and the link (type, hops) to every other visible
// device - hipExtGetLinkTypeAndHopCount; type 4 = xGMI (HSA_AMD_LINK_INFO_TYPE_XGMI), 2 = PCIe.
extern "C" int mibn_device_info(mibn_t *h, char *buf, int32_t cap) {
    if (!h || !buf || cap < 1) return MIBN_E_ARG;
    if (h->planner_only) { h->err = "planner-only context: no HIP device bound"; return MIBN_E_NODEVICE; }
    hipDeviceProp_t pr;
    HIP_TRY(h, hipGetDeviceProperties(&pr, h->device));
    char bus[64] = "?";
    (void)hipDeviceGetPCIBusId(bus, sizeof(bus), h->device);
    std::string out = "device " + std::to_string(h->device) + " " + pr.name + " (" + pr.gcnArchName + ") pci " + bus + " links:";
    int n = 0;
    (void)hipGetDeviceCount(&n);
    for (int d = 0; d < n; ++d) {
        if (d == h->device) continue;
        uint32_t type = 0, hops = 0;
        if (hipExtGetLinkTypeAndHopCount(h->device, d, &type, &hops) == hipSuccess)
            out += " ->" + std::to_string(d) + ":" + (type == 4 ? "xgmi" : type == 2 ? "pcie" : "type" + std::to_string(type)) + "/" + std::to_string(hops);
        else { (void)hipGetLastError(); out += " ->" + std::to_string(d) + ":?"; }
    }
    if (n <= 1) out += " none (one visible device)";
    std::snprintf(buf, (size_t)cap, "%s", out.c_str());
    return MIBN_OK;
}

extern "C" int mibn_comm_unique_id(mibn_t *h, void *id_out) {
    if (!h || !id_out) return MIBN_E_ARG;
    if (h->planner_only) { h->err = "planner-only context: no HIP device bound"; return MIBN_E_NODEVICE; }
    int rc;
    if ((rc = comm_load(h))) return rc;
    static_assert(sizeof(ncclUniqueId) == MIBN_COMM_ID_BYTES, "RCCL unique id size");
    ncclUniqueId id;
    NCCL_TRY(h, h->comm.GetUniqueId(&id));
    std::memcpy(id_out, &id, sizeof(id));
    return MIBN_OK;
}

extern "C" int mibn_comm_init(mibn_t *h, int32_t rank, int32_t world, const void *id_in) {
    if (!h || !id_in || world < 1 || rank < 0 || rank >= world) return MIBN_E_ARG;
    if (h->planner_only) { h->err = "planner-only context: no HIP device bound"; return MIBN_E_NODEVICE; }
    if (h->comm.comm) { h->err = "communicator already initialised"; return MIBN_E_STATE; }
    int rc;
    if ((rc = comm_load(h))) return rc;
    HIP_TRY(h, hipSetDevice(h->device));
    ncclUniqueId id;
    std::memcpy(&id, id_in, sizeof(id));
    HIP_TRY(h, h->comm.stream.ensure(hipStreamNonBlocking));
    // The collective init blocks until every rank of `world` has joined - for ever when one of them died or took another id.
    // Bounded: the call runs on a helper thread, and a rank that has waited MIBN_COMM_INIT_TIMEOUT_S seconds (default 180) gives
    // up with an error that names the likely causes instead of hanging the launch (the helper thread is abandoned: the process
    // is expected to exit on this error).
    double limit_s = 180.0;
    if (const char *e = std::getenv("MIBN_COMM_INIT_TIMEOUT_S")) { const double v = std::atof(e); if (v > 0) limit_s = v; }
    struct InitState { std::mutex m; std::condition_variable cv; bool done = false; ncclResult_t res = ncclSuccess; ncclComm_t comm = nullptr; };
    auto state = std::make_shared<InitState>();
    const int device = h->device;
    auto init_fn = h->comm.CommInitRank;
    std::thread([state, init_fn, device, world, id, rank]() {
        (void)hipSetDevice(device);
        ncclComm_t c = nullptr;
        const ncclResult_t r = init_fn(&c, world, id, rank);
        std::lock_guard<std::mutex> lk(state->m);
        state->res = r;
        state->comm = c;
        state->done = true;
        state->cv.notify_all();
    }).detach();
    {
        std::unique_lock<std::mutex> lk(state->m);
        if (!state->cv.wait_for(lk, std::chrono::duration<double>(limit_s), [&] { return state->done; })) {
            h->err = "ncclCommInitRank: rank " + std::to_string(rank) + " of " + std::to_string(world) + " on device " + std::to_string(device) +
                     " still waiting after " + std::to_string((int)limit_s) + " s (MIBN_COMM_INIT_TIMEOUT_S) - a rank died before the init, the ranks "
                     "hold different ids, two ranks share one device, or the GPUs cannot reach each other (check HSA_ENABLE_IPC_MODE_LEGACY=0)";
            return MIBN_E_COMM;
        }
        if (state->res != ncclSuccess) { h->err = std::string("ncclCommInitRank: ") + h->comm.GetErrorString(state->res); return MIBN_E_COMM; }
        h->comm.comm = state->comm;
    }
    h->comm.rank = rank;
    h->comm.world = world;
    return MIBN_OK;
}

// What RCCL itself says about the communicator (ncclCommCount / ncclCommUserRank) - not what the caller asked for: the bench
// line of an N > 1 run carries these, so that a transport that silently degraded cannot claim N ranks.
extern "C" int mibn_comm_count(mibn_t *h, int32_t *n_ranks, int32_t *my_rank) {
    int rc;
    if ((rc = comm_ready(h))) return rc;
    int n = 0, r = -1;
    NCCL_TRY(h, h->comm.CommCount(h->comm.comm, &n));
    NCCL_TRY(h, h->comm.CommUserRank(h->comm.comm, &r));
    if (n_ranks) *n_ranks = n;
    if (my_rank) *my_rank = r;
    return MIBN_OK;
}

extern "C" int mibn_comm_destroy(mibn_t *h) {
    if (!h) return MIBN_E_ARG;
    mibn_ctx::Comm &c = h->comm;
    if (c.comm) {
        (void)hipSetDevice(h->device);
        if (c.stream) (void)hipStreamSynchronize(c.stream);
        (void)c.CommDestroy(c.comm);
        c.comm = nullptr;
    }
    (void)c.stream.release();
    (void)c.d_send.release();
    (void)c.d_recv.release();
    return MIBN_OK;
}

extern "C" int mibn_comm_allgather_f64(mibn_t *h, const double *send, int64_t n, double *recv) {
    int rc;
    if ((rc = comm_ready(h))) return rc;
    if (n < 0 || (n && (!send || !recv))) return MIBN_E_ARG;
    if (n == 0) return MIBN_OK;
    mibn_ctx::Comm &c = h->comm;
    const size_t bytes = (size_t)n * 8;
    if ((rc = comm_buf(h, c.d_send, bytes))) return rc;
    if ((rc = comm_buf(h, c.d_recv, bytes * (size_t)c.world))) return rc;
    HIP_TRY(h, hipMemcpyAsync(c.d_send, send, bytes, hipMemcpyHostToDevice, c.stream));
    NCCL_TRY(h, c.AllGather(c.d_send, c.d_recv, (size_t)n, ncclDouble, c.comm, c.stream));
    HIP_TRY(h, hipMemcpyAsync(recv, c.d_recv, bytes * (size_t)c.world, hipMemcpyDeviceToHost, c.stream));
    HIP_TRY(h, hipStreamSynchronize(c.stream));
    return MIBN_OK;
}

extern "C" int mibn_comm_reduce_i64(mibn_t *h, int64_t *buf, int64_t n, int32_t root) {
    int rc;
    if ((rc = comm_ready(h))) return rc;
    mibn_ctx::Comm &c = h->comm;
    if (n < 0 || (n && !buf) || root < 0 || root >= c.world) return MIBN_E_ARG;
    if (n == 0) return MIBN_OK;
    const size_t bytes = (size_t)n * 8;
    if ((rc = comm_buf(h, c.d_send, bytes))) return rc;
    if ((rc = comm_buf(h, c.d_recv, bytes))) return rc;
    HIP_TRY(h, hipMemcpyAsync(c.d_send, buf, bytes, hipMemcpyHostToDevice, c.stream));
    NCCL_TRY(h, c.Reduce(c.d_send, c.d_recv, (size_t)n, ncclInt64, ncclSum, root, c.comm, c.stream));
    if (c.rank == root) HIP_TRY(h, hipMemcpyAsync(buf, c.d_recv, bytes, hipMemcpyDeviceToHost, c.stream));
    HIP_TRY(h, hipStreamSynchronize(c.stream));
    return MIBN_OK;
}

extern "C" int mibn_comm_allreduce_max_f64(mibn_t *h, double *buf, int64_t n) {
    int rc;
    if ((rc = comm_ready(h))) return rc;
    if (n < 0 || (n && !buf)) return MIBN_E_ARG;
    if (n == 0) return MIBN_OK;
    mibn_ctx::Comm &c = h->comm;
    const size_t bytes = (size_t)n * 8;
    if ((rc = comm_buf(h, c.d_send, bytes))) return rc;
    if ((rc = comm_buf(h, c.d_recv, bytes))) return rc;
    HIP_TRY(h, hipMemcpyAsync(c.d_send, buf, bytes, hipMemcpyHostToDevice, c.stream));
    NCCL_TRY(h, c.AllReduce(c.d_send, c.d_recv, (size_t)n, ncclDouble, ncclMax, c.comm, c.stream));
    HIP_TRY(h, hipMemcpyAsync(buf, c.d_recv, bytes, hipMemcpyDeviceToHost, c.stream));
    HIP_TRY(h, hipStreamSynchronize(c.stream));
    return MIBN_OK;
}

extern "C" int mibn_comm_barrier(mibn_t *h) {
    int rc;
    if ((rc = comm_ready(h))) return rc;
    HIP_TRY(h, hipDeviceSynchronize());  // this rank's own device work first
    double one = 1.0;
    return mibn_comm_allreduce_max_f64(h, &one, 1);
}
