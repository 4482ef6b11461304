// cx_internal.h — shared declarations of libcortex_hip.so (host side + kernel launchers).
// gfx950 only; see include/cortex_hip.h for the ABI and DESIGN.md for the data layout.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <map>
#include <memory>
#include <tuple>
#include <type_traits>
#include <string>
#include <vector>

#include "cortex_hip.h"
#include "cx_const.h"

struct cx_handle;

namespace cx {

struct ProfileRec {
    int kernel;
    hipEvent_t start, stop;
};

// One device allocation and its owner: move-only, freed by reset() and by the destructor, counted in the handle's device_bytes while
// it lives (what alloc adds, reset takes away).  Converts to T* so that launch sites read as with a raw pointer; nothing converts
// back, so a buffer cannot be assigned a pointer by accident.  alloc / upload / ensure are defined in cx_host.h (they report through
// CX_HIP like every other call).  Captured graphs hold addresses: ensure() says when the buffer moved and never drops a graph itself;
// whoever moves a buffer that a captured launch names calls cxh::captured_graphs_drop BEFORE (see upload_ptab, grow_store).
template <class T>
class DevBuf {
public:
    DevBuf() = default;
    DevBuf(DevBuf &&o) noexcept : p_(o.p_), n_(o.n_), bytes_(o.bytes_) { o.p_ = nullptr; o.n_ = 0; o.bytes_ = nullptr; }
    DevBuf &operator=(DevBuf &&o) noexcept {
        if (this != &o) { reset(); p_ = o.p_; n_ = o.n_; bytes_ = o.bytes_; o.p_ = nullptr; o.n_ = 0; o.bytes_ = nullptr; }
        return *this;
    }
    ~DevBuf() { reset(); }
    operator T *() const { return p_; }
    template <class U> explicit operator U *() const { return (U *)p_; }      // (the launchers' C casts to another element type)
    T *get() const { return p_; }
    int64_t size() const { return n_; }                                       // elements asked for (0: empty or borrowed)
    void reset() {
        if (p_ && n_) (void)hipFree((void *)p_);      // (n_ == 0: borrowed)
        if (bytes_) *bytes_ -= n_ * (int64_t)sizeof(T);
        p_ = nullptr; n_ = 0; bytes_ = nullptr;
    }
    void borrow(T *p) { reset(); p_ = p; }                                    // memory of the caller's: used, never freed or counted
    int32_t alloc(cx_handle *h, int64_t n, bool counted = true);              // a fresh buffer of max(n, 1) elements (the old one is released first)
    int32_t upload(cx_handle *h, const std::vector<T> &v);                    // alloc + asynchronous copy on the handle's stream
    int32_t ensure(cx_handle *h, int64_t n, bool *moved = nullptr);           // room for n elements; grows only, the contents are NOT kept
private:
    T *p_ = nullptr;
    int64_t n_ = 0;
    int64_t *bytes_ = nullptr;      // the owning handle's device_bytes; null: borrowed, or owned but not counted
};

template <class... B> void reset_all(B &...b) { (b.reset(), ...); }

// One instantiated graph and its owner: move-only, destroyed by reset() and by the destructor.  failed(): capture, instantiation or
// launch was refused once — plain launches from then on; reset() keeps that, only a fresh GraphExec forgets it.  Filled and launched by
// cxh::capture / cxh::launch (cx_host.h), which are the only users of get / adopt / fail.
class GraphExec {
public:
    explicit operator bool() const { return (bool)exec_; }
    bool failed() const { return failed_; }
    void reset() { exec_.reset(); }
    hipGraphExec_t get() const { return exec_.get(); }
    void adopt(hipGraphExec_t e) { exec_.reset(e); }
    void fail() { reset(); failed_ = true; }
private:
    struct Destroy { void operator()(hipGraphExec_t e) const { (void)hipGraphExecDestroy(e); } };
    std::unique_ptr<std::remove_pointer_t<hipGraphExec_t>, Destroy> exec_;
    bool failed_ = false;
};

// the stream captures are taken on: the handle's own, made on first use (cxh::capture)
struct StreamDestroy { void operator()(hipStream_t s) const { (void)hipStreamDestroy(s); } };
using OwnedStream = std::unique_ptr<std::remove_pointer_t<hipStream_t>, StreamDestroy>;

// One word of mapped host memory that a kernel raises with an ordinary store and the host reads without a copy (the paired sweep's
// abort word): move-only, freed by reset() and by the destructor.
struct HostWord {
    volatile unsigned *host = nullptr;
    unsigned *dev = nullptr;
    HostWord() = default;
    HostWord(HostWord &&o) noexcept : host(o.host), dev(o.dev) { o.host = nullptr; o.dev = nullptr; }
    HostWord &operator=(HostWord &&o) noexcept {
        if (this != &o) { reset(); host = o.host; dev = o.dev; o.host = nullptr; o.dev = nullptr; }
        return *this;
    }
    ~HostWord() { reset(); }
    void reset() { if (host) (void)hipHostFree((void *)host); host = nullptr; dev = nullptr; }
    bool alloc() {
        reset();
        void *p = nullptr, *d = nullptr;
        if (hipHostMalloc(&p, 64, hipHostMallocMapped) != hipSuccess || hipHostGetDevicePointer(&d, p, 0) != hipSuccess) {
            (void)hipGetLastError();
            if (p) (void)hipHostFree(p);
            return false;
        }
        host = (volatile unsigned *)p; dev = (unsigned *)d; *host = 0;
        return true;
    }
};

// what a handle keeps behind a pointer to a type only its own file knows (evidence, learn, sample, predict, causal, reference order): the deleter is defined there
template <class T> struct Deleter { void operator()(T *p) const; };
struct RefSched;      // cx_api_ref.hip
namespace ev { struct Cache; }
namespace evm { struct Cache; }
namespace lm { struct Cache; }
namespace fs { struct Cache; }
namespace sp { struct Plan; }
namespace pr { struct Plan; }
namespace prm { struct Plan; }
namespace cm { struct Plan; }
namespace cmm { struct Plan; }
namespace spm { struct Plan; }

}  // namespace cx

namespace cx {

// Everything a handle owns on the device for its graph, with the flags and counters that describe it.  cxh::dev_free_all assigns a
// default-constructed DevState: a member added here is freed and reset with no second mention anywhere, and the state after a reset is
// what the initialisers below say.  Assignment goes member by member in the order written here, so the captured graphs come FIRST:
// they hold the addresses of the buffers below and go before them.
// The *_dirty / *_due / *_fresh flags and the epochs below and in cx_handle: WHAT raises each of them is written in one place, cx_derived.h
// ("What a change voids"); whoever rebuilds the state a flag guards clears it where it rebuilds.
struct DevState {
    OwnedStream capture_stream;
    GraphExec tree_graph;      // CX_SCHED_TREE: the stages of one sweep as ONE graph launch (hundreds of small launches otherwise)
    // the sweeps between two exchanges of a deep-halo partition as ONE graph launch (cx_api_sweep.hip: cx_sweep): the same (first sweep after
    // the exchange, sweeps, buffers) seen a second time is captured, from then on replayed; two slots (an odd batch alternates its buffers)
    struct BatchGraph { uint64_t key = 0; GraphExec graph; int seen = 0; };
    BatchGraph batch_graph[2];
    std::unique_ptr<RefSched, Deleter<RefSched>> ref;      // CX_SCHED_REFERENCE (cx_refsched.h, cx_api_ref.hip): wiring + shadow readiness state + plans, each with its buffers and graph

    DevBuf<int32_t> d_slice_off, d_partner, d_vbase, d_var_deg;
    DevBuf<int32_t> d_big, d_big_slots, d_big_slot_var;      // (dim 2..4: the variable of every slot of the CSR tail)
    DevBuf<double2> d_big_tmp;      // prefix scratch of the big-variable kernel, one entry per big slot
    DevBuf<uint8_t> d_vinfo;
    DevBuf<double> d_q, d_a, d_b;        // per RECEIVING slot: effective rule parameters
    DevBuf<double> d_sq, d_sa, d_sb;     // the same, indexed by the SENDING slot (push)
    DevBuf<double2> d_f2v, d_v2f, d_marg;     // natural-form messages, moment-form marginals
    DevBuf<double2> d_f2v_alt;      // second factor→variable buffer (Jacobi double buffering of the fused sweep)
    DevBuf<double2> d_prev;         // snapshot for cx_residual
    DevBuf<double> d_scratch;       // small reduction scratch
    int sweep_max_w = 0;            // the widest SELL slice (0: not yet computed): picks the register footprint of the fused sweep
    DevBuf<int16_t> d_partner16;    // partner[s] - s where every difference fits (kNoPartner16: none); null otherwise (cx_kernels.hip: PACK)
    DevBuf<int32_t> d_partner_runs; // with d_partner16: {d0, d1, split, 0} per (256-slot row, wave) — cx_partner_runs.h; read by the packed k_sweep
    DevBuf<char> d_stage;           // staging for set/get/batch, in bytes (cxh::ensure_stage)
    // two sweeps per launch on a recognised grid (cx_lattice_plan.h, cx_sweep_pair.hip): the plan's shape (pair_H == 0: no plan), the rows
    // per segment (0: not chosen yet), the word a launch raises when it meets an undefined message, the flag of the definedness check
    int32_t pair_H = 0, pair_W = 0, pair_block_cols = 0, pair_rows = 0;
    std::string pair_refused;       // why the graph has no plan
    HostWord pair_abort;
    DevBuf<unsigned> d_pair_flag;
    // what pairs rely on — every variable free, every live slot of the input defined, the unary messages the same in both buffers — is
    // checked when due (raised by: cx_derived.h) and, while it does not hold, again once pair_check_at sweeps are done
    bool pair_check_due = true, pair_inputs_ok = false;
    int64_t pair_check_at = 0, pair_launches = 0;
    // three to six sweeps per launch (cx_lattice_deep.h, cx_sweep_deep.hip), in calls of at least 16 sweeps: the rows per segment of each
    // depth (indexed by depth, 3 .. 6; chosen with pair_rows; 0: not yet), the launches that ran at each depth, the depth of the last
    // call that could run them
    int32_t deep_rows[7] = {}, deep_depth = 0;      // (7 = kMaxDepth + 1: cx_api_sweep.hip asserts it)
    int64_t deep_launches[7] = {};

    // factors with more than two edges (cx_kary.hip, CX_FACTOR_GAUSS_LINEAR_N): entry = 8 * row + edge position (OUT first, then IN by
    // ascending variable id); coefficient c_e = +1 (OUT) / -a_i (IN); their slots have partner -1 (no pairwise rule touches them)
    int64_t n_kary = 0;
    std::vector<int32_t> kary_slot, slot_kary;      // [8 n_kary] slot per entry (-1 padding); [nslots] entry of a slot, -1 otherwise
    std::vector<int32_t> kary_pset;                 // dim 2..4 (cx_kary_mv.hip): [8 n_kary] parameter set of the entry — an IN entry's A, the OUT entry's Q
    DevBuf<int32_t> d_kary_pset, d_kary_v2f_slots, d_kary_v2f_vars;
    DevBuf<double> d_kary_aq;                       // [sets][2][d * d]: A | Q raw
    int64_t n_kary_v2f = 0, kary_aq_sets = 0;
    std::vector<double> kary_coef, kary_qb;         // [8 n_kary] c_e; [2 n_kary] q, b
    DevBuf<int32_t> d_kary_slot, d_slot_kary;
    DevBuf<double> d_kary_coef, d_kary_qb;
    bool kary_dirty = true;

    // multivariate path (cx_mv.hip)
    DevBuf<int32_t> d_spdir;        // per SENDING slot: 2*pset + direction of the receiving edge; -1: receiver observed
    DevBuf<double> d_ptab;          // [2*npsets][3][d*d]: (P, B, C) triples
    DevBuf<double> d_zero_msg;      // d = 64: one message of zeros (what an absent source reads)
    DevBuf<double> d_ptab_bt;       // d = 64: [2*npsets][d*d], the transposes of the B tables (cx_mv64w.hip)
    int64_t ptab_sets = 0, ptab_bt_sets = 0;      // parameter sets the device tables have room for (rewritten in place while that holds)
    DevBuf<double> d_mv_f2v, d_mv_f2v_alt, d_mv_v2f, d_mv_marg, d_mv_prev;
    int mv_max_deg = 0;             // dim 2..4: widest slice of the graph (0: not computed yet)
    // cx_set_factor_offsets (dim 2..4; cx_set_factor_offsets_mfma at the matrix-core dims: the same arrays as [nslots][d], a vector per slot,
    // h->offsets in the user's dim): x_out = A x_in + b + N(0, Q).  Allocated by the first call, for every slot, and rewritten in place
    // from then on (a captured sweep holds d_off_g by value): the offset of each slot's factor, [d][nslots]; the linear term it puts at
    // the slot's end, [d][nslots] (k_mv_offset_terms, again after cx_set_factor_matrices); the rule table of the messages INTO each slot
    DevBuf<double> d_off_b, d_off_g;
    DevBuf<double> d_off_kappa;     // the matrix-core dims: b'Q⁻¹b of each slot's factor, [nslots] (k_offset_terms64; the evidence reads it)
    DevBuf<int32_t> d_off_rt;
    // d = 64 work lists (built lazily: they depend on which variables are observed)
    bool work64_dirty = true, point64_dirty = true;
    DevBuf<int32_t> d_point64_slots;
    DevBuf<int32_t> d_rule64_rec;   // 8 words per work item (see k_rule64)
    // senders of degree 5 .. 8 (a rule sums at most three sources): their variable→factor messages are summed first (k_v2f64) and the
    // rule reads the stored message; the same per stage of the tree schedule
    int64_t n_pre64 = 0;
    DevBuf<int32_t> d_pre64_slots, d_pre64_vars, d_tree_pre_slots, d_tree_pre_vars;

    // CX_SCHED_TREE (cx_tree_plan.h): the stages' items and k-ary entries, the stage table (runs of thin stages go out as one launch)
    bool chains_dirty = true, tree_dirty = true;
    DevBuf<int32_t> d_tree_rec, d_tree_kary;
    DevBuf<int64_t> d_tree_stage_off;
    // the same sweep over heavy paths (cx_tree_plan.h: build_hp), chosen when it takes fewer launches: the paths' arrays live in the chain
    // fields (d_chain_pos_var .. d_chain_totals; d_chain_skip1 is the way up's), item stages in d_tree_rec as before
    bool tree_hp = false;
    DevBuf<int32_t> d_tree_skip1_down;
    // heavy paths through factors with more than two edges: their pairwise parameters per receiving slot are written every sweep
    // (cx_kary.hip: k_kary_link_params) into d_q and into d_a / d_b — or, on a graph without pairwise linear factors, into these
    DevBuf<double> d_tree_a, d_tree_b;

    // chain-scan schedule (cx_chain.hip)
    DevBuf<int32_t> d_chain_pos_var, d_chain_skip0, d_chain_skip1;
    DevBuf<int32_t> d_chain_link_pos, d_chain_from, d_chain_to;
    // dim 1: the slots that send into a non-observed variable of degree 1 (a forecast's last state): it is off the chains, and the
    // message into it is the rule applied to a variable→factor message that exists only once the scan has run (sweep_main)
    DevBuf<int32_t> d_chain_leaf_from;
    int64_t chain_nleaf = 0;
    DevBuf<uint8_t> d_chain_head_fwd, d_chain_head_bwd;
    DevBuf<double2> d_chain_side;
    DevBuf<char> d_chain_totals;    // bytes: the tile totals of whichever scan the dim runs
    // dim 2..4 (cx_mvchain.hip): rule-table index of each link's two messages, side sums [nc][npos], tile totals of the map scan
    DevBuf<int32_t> d_chain_tab_fwd, d_chain_tab_bwd;
    DevBuf<double> d_mvc_side, d_mvc_totals;
    DevBuf<int32_t> d_mvc_var_link;      // per variable: the chain link whose RIGHT end it is, -1 otherwise (dim 2..4; marginals on demand)
    DevBuf<double> d_mvc_side_l, d_mvc_alpha, d_mvc_gamma, d_mvc_prefix, d_mvc_wave_carry, d_mvc_block;   // thread-interleaved by link, [nc][ntiles * 256 * K]

    // halo: the lists, and the pack / unpack buffers — the handle's own, or the caller's (cx_halo_set_buffers: DevBuf::borrow)
    DevBuf<int32_t> d_send_slots, d_recv_slots, d_send_vars;
    DevBuf<double2> d_send_buf, d_recv_buf;

    // cx_set_messages of a long list the caller repeats: see cx_handle::set_memo_tick
    struct SetMemo { uint64_t key = 0, used = 0; int32_t direction = 0; std::vector<int64_t> var_ids, fac_ids, edges; std::vector<int32_t> idx, vars; };
    std::vector<SetMemo> set_memos;

    // stores of the batched API's intermediates: ProductOfMessages nodes (variable, lo, hi) and JointMarginal nodes (factor); the
    // stores hold size() entries (multiples of 256)
    std::map<std::tuple<int32_t, int32_t, int32_t>, int32_t> prod_index;
    std::map<int32_t, int32_t> joint_index;
    DevBuf<double2> d_prod;
    DevBuf<double> d_joint;
    DevBuf<double> d_mv_prod;       // dim > 1: the ProductOfMessages table (natural form; dim 2..4 in the messages' pair form, dim 64 one row of 4,160 doubles each)
    int64_t mv_prod_cap = 0;        // entries it holds (a multiple of 256)

    // the XCD-resident cluster (cx_api_ref.hip: cluster_prepare)
    DevBuf<char> d_cluster_ctl;     // 512 B the launch scribbles on (cx_batch.hip: ClusterCtl)
    int cluster_state = 0;          // 0 not prepared, 1 ready, -1 off (CX_REF_CLUSTER=0, no memory, another architecture, or a barrier once timed out)

    // cx_log_evidence (cx_evidence.hip): work lists of the graph and scratch, built on the first call; cx_factor_beliefs /
    // cx_factor_statistics (cx_learn.hip): the grouping's work lists and scratch; cx_sample_posterior (cx_sample.hip): the forest
    // plan, the links and the per-call scratch; cx_predictive (cx_predict.hip): the rows of the last (mode, factor_ids) and their scratch
    std::unique_ptr<ev::Cache, Deleter<ev::Cache>> evidence;
    // cx_log_evidence_mfma (cx_evidence_mfma.hip): the term lists of the matrix-core dims, the log-det table and the call's scratch
    std::unique_ptr<evm::Cache, Deleter<evm::Cache>> evidence_mfma;
    // cx_factor_beliefs_mfma / cx_factor_statistics_mfma (cx_learn_mfma.hip) and cx_factor_disturbances_mfma (cx_disturb_mfma.hip): the factor
    // records, the grouping's partials, the disturbances' rows and the workspace
    std::unique_ptr<lm::Cache, Deleter<lm::Cache>> learn_mfma;
    std::unique_ptr<fs::Cache, Deleter<fs::Cache>> learn;
    std::unique_ptr<sp::Plan, Deleter<sp::Plan>> sample;
    std::unique_ptr<pr::Plan, Deleter<pr::Plan>> predict;
    // cx_predictive_mfma (cx_predict_mfma.hip): the rows of the last (mode, factor_ids) at the matrix-core dims, the [A' | Q] table and the call's scratch
    std::unique_ptr<prm::Plan, Deleter<prm::Plan>> predict_mfma;
    // cx_causal_marginals_mfma (cx_causal_mfma.hip): the rows of the last (mode, lag > 0 or not, variable_ids) at the matrix-core dims, the
    // transition entries of the fixed-lag recursion and the call's scratch (the β buffers among it, allocated by the first call with a lag)
    std::unique_ptr<cmm::Plan, Deleter<cmm::Plan>> causal_mfma;
    // cx_sample_posterior_mfma (cx_sample_mfma.hip): the forest plan of cx_sample_core.h with the link records of the matrix-core dims,
    // the link workspace (2 KD² + KD doubles per free variable: it stays across a rebuild of the plan) and the call's scratch
    std::unique_ptr<spm::Plan, Deleter<spm::Plan>> sample_mfma;
    // cx_causal_marginals (cx_causal.hip): the class of every slot and the transition list, with the call's scratch; the plan is due
    // again after whatever changes the graph or the observed flags (raised by: cx_derived.h)
    std::unique_ptr<cm::Plan, Deleter<cm::Plan>> causal;
    bool causal_plan_dirty = true;
};

}  // namespace cx

// The raw exceptions.  The launchers that live in the profiled kernel sources (build.py: KERNEL_SOURCES) assign or take the address of
// d_chain_linkpar, d_chain_onepass, d_chain_abort (cx_chain.hip), d_marg64_sums, d_marg64_tab, d_marg64_rec (cx_mv64.hip) and own the
// chain64 (cx_mv64chain.hip) and vmp (cx_vmp.hip) sub-states; an edit of those files' code would void the counter profiles kept
// under profiles/, so these stay raw pointers of cx_handle, freed where they always were (chain_onepass_free, chain64_free,
// chain64_tree_free, vmp_free, dev_free_all for the three d_marg64_*).  Everything else a handle owns on the device is in DevState,
// the captured graphs (cx::GraphExec) and the stream they are captured on included.
struct cx_handle : cx::DevState {
    cx_config cfg{};
    std::string err;
    hipStream_t stream = nullptr;
    bool has_graph = false;

    // ---- host copy of the flattened graph (lookup + batching) ----
    int64_t nv = 0, nf = 0, ne = 0;     // variables, factors, connections
    int64_t nslots = 0;                 // message slots (SELL region incl. padding + big-variable CSR region)
    int64_t nslices = 0;
    std::vector<int64_t> var_ids;       // ascending; index = local variable number
    std::vector<int64_t> fac_ids;       // ascending; index = local factor number
    std::vector<int32_t> fac_kind;      // by local factor number
    std::vector<double> fac_params;     // [nf][CX_NPARAM]
    std::vector<int32_t> var_off;       // [nv+1] CSR offsets into the edge table sorted by (variable id, factor id)
    std::vector<int64_t> edge_fac_id;   // [ne] factor id per CSR edge
    std::vector<int32_t> edge_var;      // [ne] local variable number per CSR edge
    std::vector<int32_t> vbase;         // [nv] slot of the variable's first message
    std::vector<uint8_t> vinfo;         // [nv] degree class + flags
    std::vector<int32_t> slice_off;     // [nslices+1] first slot of each slice
    std::vector<int32_t> partner;       // [nslots] slot of the other edge of a 2-edge factor, -1 otherwise
    std::vector<int32_t> big_vars;      // variables with degree > kSmallDeg
    std::vector<int32_t> big_slots;     // all slots of big variables (the fused schedule pushes them separately)
    int64_t n_messages_per_sweep = 0;
    int64_t sweeps_done = 0;
    bool any_linear = false;

    // ---- device buffers ----
    int32_t big_start = 0;          // first slot of the big-variable CSR tail
    // chain scan, set by an owner that drives this handle (cx_vmp.hip's inner handle; never owned here):
    const int32_t *d_q_gamma = nullptr;   // per slot: index into d_q_gmean of the precision variable whose mean sets this factor's variance
    const double *d_q_gmean = nullptr;    //   q = 1 / d_q_gmean[d_q_gamma[slot]] read in place of d_q[slot] (no per-slot table to rewrite per call)
    double *d_split_mean = nullptr, *d_split_prec = nullptr;   // the scan writes (mean, precision) of the chain variables here instead of d_marg
    bool split_marg_written = false;      // ... and did so in the last sweep
    bool pot64_fresh = false;             // dim 64, a partition's time block: the potentials of the composition tree are those of the data on the device
                                          // (cx_chain_block_maps just composed them and nothing they read has changed): the next sweep starts at its walks
    int32_t pot64_end_slots[6] = {-1, -1, -1, -1, -1, -1};      // side slots of the path's two END positions: no composition reads them
    bool chain_msgs_unread = false;       // the owner reads the chain links' variable→factor messages and marginals only: the scan need not store
                                          // the factor→variable messages of the links (nothing of this handle is asked for them)
    int64_t device_bytes = 0;       // the sum of the live DevBufs of this handle (+ what the raw exceptions below added)

    // multivariate path (cx_mv.hip), dim in {2,3,4}: SoA component-major buffers [nc][nslots], packed symmetric Lambda
    int nc = 2;                                    // doubles per message (eta + packed Lambda; 64 + 64*64 for dim 64)
    int ncs = 2;                                   // STORED doubles per message slot: dim 2..4 pad nc to whole 16-byte pairs (cx_mv_core.h)
    std::vector<std::vector<double>> psets;        // per parameter set: A (d*d) then Q (d*d)
    std::vector<int32_t> spdir;                    // host copy without the observed-receiver mask
    bool spdir_dirty = true;
    int observed_passes_due = 2;                   // sweeps that still have to write the messages out of observed variables
    // dim 16 / 32: the marginal read-out's scratch (sums of the listed variables' messages + their rule records) and identity table
    double *d_marg64_sums = nullptr, *d_marg64_tab = nullptr;
    int32_t *d_marg64_rec = nullptr;
    int64_t marg64_cap = 0;
    int64_t max_pset = -1;
    int64_t n_rule64 = 0, n_point64 = 0;           // d = 64 work lists (DevState: d_rule64_rec, d_point64_slots)
    std::vector<int64_t> tree_pre_off;

    // chain-scan schedule (cx_chain.hip): paths of free variables, built lazily by build_chains()
    // cfg.dim of 5 .. 63 as the caller gave it (0 otherwise): such a handle runs as dim 64 with every message, datum and rule matrix
    // embedded block-diagonally (cx_api.hip: pad_* helpers); cfg.dim holds 64
    int user_dim = 0;
    // CX_SCHED_TREE (cx_tree_plan.h): the stages' items and k-ary entries on the device (DevState), their offsets on the host
    std::vector<int64_t> tree_stage_off, tree_kary_off;
    int64_t tree_stats[8] = {0, 0, 0, 0, 0, 0, 0, 0};      // depth, stages, items, k-ary entries, components, up, down, marginals
    // the same sweep over heavy paths (DevState: tree_hp)
    std::vector<int32_t> tree_hp_steps;            // pairs (kind, index): 0 item stage, 1 scan of a light depth on the way up, 2 its final scan
    std::vector<int64_t> tree_hp_pos_off, tree_hp_link_off;
    int32_t tree_hp_marginal_stage = -1;
    int64_t tree_hp_stats[4] = {0, 0, 0, 0};       // light depths, paths of two or more, variables on no such path, launches per sweep
    int64_t tree_hp_kary_links = 0;
    // dim 2 .. 4 over heavy paths: the scans of cx_mvchain.hip on a light depth's range; links per thread chosen per depth, the
    // interleaved buffers (d_mvc_*) sized for the largest depth and shared by all of them
    std::vector<int32_t> tree_hp_K;
    int64_t tree_hp_npos = 0;
    // dim 64 over heavy paths: a plan of compositions and walks (cx_chain64_plan.h) per light depth and direction of travel
    std::vector<void *> tree_c64;
    std::vector<int32_t> tree_c64_up, tree_c64_final;      // per light depth: index into tree_c64, -1 = no such scan
    int64_t chain_npos = 0, chain_nlinks = 0;
    int64_t chain_npos_linked = 0;   // dim > 1: positions [0, this) belong to paths with links; the isolated ones follow
    bool chain_side_dirty = true;    // the leaf messages / side sums of the chain positions are due (raised by: cx_derived.h)
    bool chain_partition = false;    // the handle holds a time block of a partitioned chain (cx_chain_block_maps was called)
    bool chain_covers_all = false;   // every variable that reads messages is a chain position: the scan's side pass produces all leaf messages
    uint64_t batch_epoch = 1;        // deep-halo batch graphs (DevState: batch_graph): moved on by whatever a captured batch bakes in (layers, damping, the graph itself): cxh::batch_graph_drop
    int64_t batch_graph_launches = 0;
    // the chain scan as ONE launch (cx_chain.hip: k_chain_onepass): tile totals + flags on the device, the word in mapped host memory that a
    // workgroup raises when a wait of it times out (checked by every CX_HIP of the host: the call that finds it fails, the handle goes back to two launches)
    void *d_chain_onepass = nullptr, *d_chain_abort = nullptr;
    volatile unsigned *chain_abort_host = nullptr;
    // the chain links' rule parameters in link order (cx_chain.hip: k_chain_linkpar); chain_pos0 >= 0: link l's left end is position chain_pos0 + l
    void *d_chain_linkpar = nullptr; int64_t chain_linkpar_cap = 0; bool chain_linkpar_dirty = true; const void *chain_linkpar_qg = nullptr; int chain_pos0 = -1;
    int chain_onepass_state = 0, chain_onepass_cus = 0;      // 0 not prepared, 1 ready, -1 off (CX_CHAIN_ONEPASS=0, no memory, or a wait once timed out)
    int64_t chain_onepass_launches = 0;
    bool mvc_marg_pending = false;      // dim 2..4 chain scan, compute_marginals_in_sweep == 2: the last sweep left alpha and gamma, the marginals are formed when read
    int mvc_K = 4;                   // links per thread of the scan (fixed when the chains are built)
    void *chain64 = nullptr;         // dim 64 chain scan (cx_mv64chain.hip): the plan's records, potential and entry arenas on the device
    bool chain_msgs_stale = false;   // dim 2..4 chain scan: the chain messages in d_mv_f2v are older than the last sweep (refreshed on demand)

    // halo
    std::vector<int32_t> send_slots, recv_slots;
    bool halo_state = false;         // halo lists name factor→variable messages of redundant variables (deep halo)
    // deep halo: redundant layer of each variable (cx_halo_set_layers) -> slice range that sweep j after an exchange has to run
    int halo_depth = 0, sweeps_since_exchange = 0;
    std::vector<int32_t> trim_lo, trim_hi;   // [depth + 1]: first / last slice holding a variable of layer <= L
    int run_slice0 = 0, run_nslices = 0;     // what launch_fused covers (0 slices: everything)
    int run_excl_lo = 1, run_excl_hi = 0;    // ... minus this slice range (empty by default)
    int64_t partner_run_entries = 0, partner_run_fallback = 0, sweeps_without_marginals = 0;      // cx_sweep_stats
    bool run_skip_marg = false;              // cx_sweep sets it around every sweep of a call but the last: nobody can read that sweep's marginals
    int own_slice_lo = 1, own_slice_hi = 0;  // deep halo: the run of slices that hold OWNED variables only (cx_halo_set_layers); empty: none
    // RCCL exchange issued by the library (cx_comm.hip)
    struct Peer { int rank; int64_t send_off, send_count, recv_off, recv_count; };
    std::vector<Peer> peers;
    void *comm = nullptr;            // ncclComm_t
    int comm_world = 0, comm_rank = -1;
    hipStream_t comm_stream = nullptr;
    hipEvent_t ev_packed = nullptr, ev_recv = nullptr, ev_swept = nullptr;
    // deep-halo exchange through IPC-mapped receive areas and epoch flags (cx_api_ipc.hip)
    struct IpcConn { void *opened = nullptr; void *mapped = nullptr; char handle[64] = {0}; unsigned long long *flag = nullptr; double2 *area[2] = {nullptr, nullptr}; bool connected = false; };
    std::vector<IpcConn> ipc_conn;   // one per peer entry: where this rank pushes
    // raw on purpose: the block comes from hipExtMallocWithFlags and is exported to the peers, whose mapped views are not ours to free;
    // both are made and freed by cx_api_ipc.hip alone (ipc_destroy), apart from the graph's memory and uncounted
    void *d_ipc_block = nullptr;     // this rank's flags + two receive areas (fine-grained, exported)
    void *d_ipc_local = nullptr;     // push completion counter, error word
    int64_t ipc_area_bytes = 0, ipc_epoch = 0, ipc_pushed = 0;   // epochs unpacked / pushed
    double ipc_timeout_s = 20.0;
    bool ipc_fused = false;          // cx_halo_ipc_set_fused: push and unpack of an exchange as ONE launch (every neighbour pushes from another device)
    int ipc_quiet_lo = 1, ipc_quiet_hi = 0;   // the longest run of owned-only slices none of whose variables WRITES a message of the send list
                                              // (cx_halo_ipc_batch: that run of the last sweep is computed after the push); empty: none
    // cx_set_factor_offsets was called (the sweeps then launch the kernels' OFF instances); whether any offset is non-zero; the offsets
    // by local factor number, [nf][d]; the two slots of every factor (-1: none), built by the first call
    bool has_offsets = false, offsets_nonzero = false;
    std::vector<double> offsets;
    std::vector<int32_t> off_fac_slots;
    double damping = 0.0;            // cx_set_damping: new = (1 - damping) rule + damping old (fused and flooding sweeps)
    // cx_set_messages of a long list the caller repeats (an iteration re-sets its priors before every call): ids -> slots / variables / edges,
    // kept for the last lists (the ids themselves are kept and compared: a hash alone would be trusted with the device's memory)
    uint64_t set_memo_tick = 0;
    uint64_t vinfo_epoch = 0;        // the observed flags of vinfo changed (cx_derived.h); read by ref_sweep_all's cached "every free variable" request
    bool in_sweep = false;
    bool v2f_stale = false;          // fused schedule without materialisation: v2f must be recomputed before use
    bool chain_v2f_from_scan = false; // the scan also stores the variable→factor messages of the chain links (set by cx_vmp.hip on its inner handle)
    bool offchain_marg_dirty = true; // scalar chain scan: marginals of variables OFF the chains (observed, stand-ins) are due (cx_derived.h)

    // stores of the batched API's intermediates: ProductOfMessages nodes (variable, lo, hi) and JointMarginal nodes (factor)
    std::vector<uint8_t> lin_out_is_second;   // per factor (GAUSS_LINEAR): the OUT edge is the edge of the higher variable id
    std::vector<int8_t> np_role;              // per CSR edge: the role on a CX_FACTOR_NORMAL_PRECISION factor, -1 elsewhere (empty: no such factor)
    std::vector<uint8_t> var_gamma;           // per variable: 1 = the precision of such factors, Gamma-distributed (marginal stored as (shape, scale))
    std::vector<int32_t> fac_edges;           // [2 nf] CSR edges of each (≤ 2-edge) factor, built on first use

    // the XCD-resident cluster (cx_batch.hip: k_ref_cluster; cx_api_ref.hip: cluster_prepare / cluster_run): stage plans of wide stages in ONE launch
    int cluster_cu = 0;              // compute units = workgroups of a cluster launch
    int64_t cluster_recoveries = 0;  // calls whose cluster gave up at a barrier and that were finished on plain launches (cx_cluster_stats)
    std::string cluster_note;        // what happened, for cx_last_error's reader
    int64_t cluster_max_items = 16384, cluster_min_items = 128;      // a stage wider than max (one pass of the members) is a launch of its own on the whole chip; plans of fewer than min items per stage are chains

    // CX_SCHED_REFERENCE (DevState: ref): the list of the plan being launched, an alias into that plan (cx_batch.hip reads it)
    int32_t *d_ref_list = nullptr;

    // variational families (cx_vmp.hip): opaque state
    void *vmp = nullptr;

    // moves on with every change of rule parameters (cx_derived.h: Change::Rule*); the parameter part of the evidence and learn caches follows it
    uint64_t param_epoch = 0;

    // profiling
    bool profiling = false, prof_armed = false;
    hipStream_t prof_stream = nullptr;
    int prof_stride = 1;
    int64_t prof_count[CX_KERNEL_COUNT] = {0};
    std::vector<cx::ProfileRec> recs;
};

namespace cx {

// slot of CSR edge e (host)
// the distance between two consecutive slots of variable v: 1 in the CSR tail (degree > 8), 256 in a slice
inline int32_t slot_stride(const cx_handle *h, int32_t v) { return ((h->vinfo[v] & kDegMask) == kBigDeg) ? 1 : kBlock; }
inline int32_t slot_of_edge(const cx_handle *h, int64_t e) {
    const int32_t v = h->edge_var[e];
    const int32_t k = (int32_t)(e - h->var_off[v]);
    return ((h->vinfo[v] & kDegMask) == kBigDeg) ? h->vbase[v] + k : h->vbase[v] + k * kBlock;
}

// kernel launchers (cx_kernels.hip)
void launch_fused(cx_handle *h, const double2 *f2v_in, double2 *f2v_out, bool write_marg, bool store_v2f, bool skip_ghosts);
void launch_var_to_factor(cx_handle *h, const double2 *f2v, bool write_marg);
void launch_big_var_to_factor(cx_handle *h, const double2 *f2v, bool write_marg);
void launch_factor_to_var(cx_handle *h, const double2 *v2f, double2 *f2v);
void launch_push_slots(cx_handle *h, const int32_t *d_slots, int64_t n, double2 *f2v_out, int kernel_id);
void launch_halo_export(cx_handle *h, const double2 *f2v, hipStream_t stream);
void launch_halo_import(cx_handle *h, double2 *f2v_out, bool push);
void launch_batch(cx_handle *h, const int32_t *d_rec, int64_t n);
void launch_flat_run(cx_handle *h, const int32_t *d_flat, const int32_t *d_rec, const int64_t *d_stage_off, int s0, int s1);
int flat_run_max();      // stages of at most this many records   // launch_batch_run on flat records
void launch_ref_cluster(cx_handle *h, void *d_ctl, int n_workgroups, const int32_t *d_flat, const int32_t *d_rec, const int64_t *d_stage_off, int n_stages);   // all stages behind single-XCD barriers; ctl[4] != 0 afterwards: a wait timed out
void launch_wide_sum(cx_handle *h, const int32_t *d_rec, int64_t n, void *d_partial);   // reference plans: list items of more than cx::refsched::kWideList sources, a workgroup each
void launch_batch_run(cx_handle *h, const int32_t *d_rec, const int64_t *d_stage_off, int s0, int s1);   // consecutive thin stages (<= 1024 items each) in one launch
constexpr int kSmallBatch = 48;                        // items whose records (5 int32 each) ride in the kernel arguments
struct SmallBatch { int32_t r[5 * kSmallBatch]; };
void launch_batch_small(cx_handle *h, const SmallBatch &recs, int n);   // 5 int32 per item: kind, index, var, lo, hi
void launch_scatter(cx_handle *h, double2 *dst, const int32_t *d_idx, const double2 *d_val, int64_t n);
void launch_gather(cx_handle *h, const double2 *src, const int32_t *d_idx, double2 *d_val, int64_t n);
void launch_seed(cx_handle *h, double2 *buf, int64_t n, double2 value, const int32_t *partner);
// factors with more than two edges (cx_kary.hip)
int32_t kary_upload(cx_handle *h);
void launch_kary(cx_handle *h, const double2 *v2f, double2 *f2v_out);
void launch_kary_items(cx_handle *h, const int32_t *d_entries, int64_t n);
void launch_kary_link_params(cx_handle *h, int64_t link_lo, int64_t nlinks, double *a, double *b);
// the same factors for dim 2..4 (cx_kary_mv.hip)
int32_t kary_mv_upload(cx_handle *h);
void mv_launch_kary(cx_handle *h, double *f2v_out = nullptr);
void launch_residual(cx_handle *h, const double2 *cur, const double2 *prev, int64_t n, double *d_out);
// two sweeps per launch on a grid (cx_sweep_pair.hip)
int64_t pair_capacity_blocks(const cx_handle *h);
void launch_sweep_pair(cx_handle *h, const double2 *f2v_in, double2 *f2v_out);
void launch_pair_check(cx_handle *h, const double2 *f2v, const double2 *alt, unsigned *d_flag);
int64_t deep_capacity_blocks(const cx_handle *h, int depth);      // cx_sweep_deep.hip: depth 3 .. 6 (cx_lattice_deep.h: kMaxDepth)
void launch_sweep_deep(cx_handle *h, int depth, const double2 *f2v_in, double2 *f2v_out);
void launch_chain_scan(cx_handle *h, double2 *f2v, bool fused_leaves, int marg_form, bool chain_v2f);
void launch_chain_totals(cx_handle *h, double2 *f2v, bool fused_leaves, int64_t *ntiles_out);
void launch_chain_scan_range(cx_handle *h, double2 *f2v, int64_t pos_lo, int64_t npos, int64_t link_lo, int64_t nlinks, const int32_t *skip1, bool final);
// multivariate (cx_mv.hip)
void mv_launch_sweep(cx_handle *h, bool write_marg, int only, double *f2v_out = nullptr);   // only: 0 regular, 1 observed variables, 2 other fixed senders (degree 1, stand-ins)
void mv_launch_v2f(cx_handle *h, const int32_t *d_slots, const int32_t *d_vars, int64_t n, const double *f2v);
void mv_launch_big(cx_handle *h, bool write_marg, double *f2v_out = nullptr);     // the variables of degree > 8 of a fused sweep (dim 2..4)
void mv_launch_scatter(cx_handle *h, double *dst, int64_t stride, int nc, int ncs, const int32_t *d_idx, const double *d_val, int64_t n);
void mv_launch_gather(cx_handle *h, const double *src, int64_t stride, int nc, int ncs, const int32_t *d_idx, double *d_val, int64_t n);
void mv_launch_seed(cx_handle *h, double *buf, double eta, double lam);
void mv_launch_batch_small(cx_handle *h, const SmallBatch &recs, int n);
void mv_launch_batch_run(cx_handle *h, const int32_t *d_rec, const int64_t *d_stage_off, int s0, int s1);   // stages [s0, s1), each at most mv_run_block() items, one workgroup
int mv_run_block();
void mv_launch_batch(cx_handle *h, const int32_t *d_rec, int64_t n);   // cx_mvbatch.hip: 5 int32 per item (kind, index, variable, rule table, 0)
void mv_launch_residual(cx_handle *h, const double *cur, const double *prev, int64_t n, double *d_out);
void mv_launch_offset_terms(cx_handle *h);      // cx_set_factor_offsets: d_off_b and the rule tables -> d_off_g
bool spd_inverse(int d, const double *S, double *out);
// d = 64 (cx_mv64.hip): message-major layout, MFMA rule kernel
void mv64_launch_rule(cx_handle *h, int nwork, const int32_t *d_rec, const double *f2v_in, double *f2v_out, int kernel_id);
void mv64w_launch_rule(cx_handle *h, int nwork, const int32_t *d_rec, const double *f2v_in, double *f2v_out);   // cx_mv64w.hip
void mv64_launch_marginals(cx_handle *h, int n, const int32_t *d_vars, const double *f2v, double *out);
void mv64w_launch_marginal_rule(cx_handle *h, int n, const int32_t *d_rec, const double *ident_tab, const double *ident_bt, const double *sums, double *out);
void mv64_launch_point(cx_handle *h, int nwork, const int32_t *d_slots, double *out_a, double *out_b);
void mv64_launch_offset_terms(cx_handle *h);      // cx_set_factor_offsets_mfma: d_off_b and the rule tables -> d_off_g, [nslots][d]
void mv64_launch_v2f(cx_handle *h, int n, const int32_t *d_slots, const int32_t *d_vars, const double *f2v);
void mv64_launch_damp(cx_handle *h, int n, const int32_t *d_rec, const double *old, double *out, double lam);
void mv64_launch_range_sums(cx_handle *h, int n, const int32_t *d_rec4, const double *f2v, double *out);      // rec: destination row, n sources, first slot, slot stride
void mv64_launch_seed(cx_handle *h, double *buf, double eta, double lam);
void mv64_rows_scatter(cx_handle *h, double *dst, const int32_t *d_idx, const double *d_val, int64_t n);
void mv64_rows_gather(cx_handle *h, const double *src, const int32_t *d_idx, double *d_val, int64_t n);
void mv64_set_point(cx_handle *h, double *dst, const int32_t *d_idx, const double *d_y, int64_t n);
bool mv_rule_tables(int d, const double *A, const double *Q, double *out);
size_t chain_total_bytes(int64_t nlinks);
void chain_onepass_free(cx_handle *h);
// chains inside reference-order plans as scans (cx_planscan.hip)
int64_t plan_scan_scratch_bytes(int64_t nlinks);
int64_t plan_scan_max_links();
void launch_plan_scan(cx_handle *h, const int32_t *lead_dst, const int32_t *lead_var, const int32_t *fol_dst, const int32_t *prec, const int32_t *src_off,
                      const int32_t *src, const uint8_t *head, int64_t lo, int64_t hi, void *scratch);
// chain scan for dim 2..4 (cx_mvchain.hip)
int mvc_links_per_thread(int64_t nlinks);
size_t mvc_prefix_doubles(int dim, int64_t nlinks, int K);
size_t mvc_wave_carry_doubles(int dim, int64_t nlinks, int K);
int64_t mvc_ntiles(int64_t nlinks, int K);
size_t mvc_totals_doubles(int dim, int64_t nlinks, int K);
void mvc_launch_side(cx_handle *h, bool write_marg);
void mvc_launch_scan(cx_handle *h, bool write_marg, bool store_msgs, bool scan, bool defer_marg = false);
void mvc_launch_scan_range(cx_handle *h, int64_t npos_total, int64_t pos_hi, int64_t link_lo, int64_t nlinks, int K, const int32_t *skip1, bool final);
void mvc_launch_marg_out(cx_handle *h);
void mvc_launch_marg_gather(cx_handle *h, const int32_t *d_vars, int64_t n, double *d_val);   // a few marginals from alpha + gamma (rows of nc doubles, moment form, packed)      // alpha + gamma of the last sweep -> the marginals (what a sweep with defer_marg left undone)
void mvc_launch_block_maps(cx_handle *h);
// chain scan for dim 64 (cx_mv64chain.hip; the plan: cx_chain64_plan.h)
int32_t chain64_build(cx_handle *h, const std::vector<int32_t> &pos_var, const std::vector<int32_t> &skip0, const std::vector<int32_t> &skip1,
                      const std::vector<int32_t> &link_pos, const std::vector<int32_t> &from, const std::vector<int32_t> &to,
                      const std::vector<uint8_t> &head_fwd, const std::vector<uint8_t> &head_bwd, const std::vector<int32_t> &tab_fwd,
                      const std::vector<int32_t> &tab_bwd);
int32_t chain64_sweep(cx_handle *h);
void chain64_free(cx_handle *h);
int32_t chain64_tree_build(cx_handle *h, int *index, const std::vector<int32_t> &pos_var, const std::vector<int32_t> &skip0, const std::vector<int32_t> &skip1,
                           const std::vector<int32_t> &link_pos, const std::vector<int32_t> &from, const std::vector<int32_t> &to,
                           const std::vector<uint8_t> &head_fwd, const std::vector<uint8_t> &head_bwd, const std::vector<int32_t> &tab_fwd,
                           const std::vector<int32_t> &tab_bwd);
int32_t chain64_tree_resolve(cx_handle *h);
int64_t chain64_tree_launches(const cx_handle *h, int index);
int32_t chain64_tree_sweep(cx_handle *h, int index);
void chain64_tree_free(cx_handle *h);
void chain64_stats(const cx_handle *h, int64_t *out8);
int32_t chain64_block_potential(cx_handle *h, double *pot, int32_t *side_first3, int32_t *side_last3, bool *no_root);
// variational families (cx_vmp.hip)
int32_t vmp_graph_create(cx_handle *h, int64_t ne, const int64_t *edge_var, const int64_t *edge_fac, const int32_t *edge_role,
                         int64_t nf, const int64_t *factor_ids, const int32_t *factor_kind);
int32_t vmp_set_marginals(cx_handle *h, int64_t n, const int64_t *ids, int32_t form, const double *payload);
int32_t vmp_get_marginals(cx_handle *h, int64_t n, const int64_t *ids, double *out);
int32_t vmp_update_marginals(cx_handle *h, int64_t n, const int64_t *ids);
int32_t vmp_set_stream(cx_handle *h);
int32_t vmp_state_bytes(cx_handle *h, int64_t *bytes);
int32_t vmp_state_export(cx_handle *h, void *buf, int64_t bytes);
int32_t vmp_state_import(cx_handle *h, const void *buf, int64_t bytes);
void vmp_free(cx_handle *h);
// RCCL halo exchange (cx_comm.hip)
bool comm_unique_id(void *out128, std::string &err);
bool comm_init(cx_handle *h, int world, int rank, const void *id128, std::string &err);
void comm_destroy(cx_handle *h);
bool comm_exchange(cx_handle *h, std::string &err, bool packed_on_comm_stream);
bool comm_exchange_on(cx_handle *h, hipStream_t stream, std::string &err);
void ipc_destroy(cx_handle *h);  // cx_api_ipc.hip

}  // namespace cx
