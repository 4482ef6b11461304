/*
 * cortex_hip.h — C ABI of libcortex_hip.so: the MI355X (gfx950) sum-product sweep that sits
 * behind Cortex.jl's InferenceEngine / AbstractInferenceRequestProcessor plugin API.
 *
 * The reference (Cortex.jl v0.3.0, pure Julia) has no FFI; these entry points are what a Julia
 * `ccall` shim for this path binds (INTEGRATION.md shows the stub).  Each declaration names the
 * reference interface it replaces (paths relative to the reference checkout):
 *
 *   graph ingestion      the 7 model-engine accessors, src/model_engine.jl:329-391, as forwarded by
 *                        ext/BipartiteFactorGraphsExt/BipartiteFactorGraphsExt.jl:16-48
 *   cx_set_messages      set_value!(message, data)                         src/signal.jl:232-253
 *   cx_update_batch      process!(processor, engine, variable_id, signal)  src/inference_engine.jl:479-509
 *                        → compute_message_to_variable! / compute_message_to_factor! /
 *                          compute_individual_marginal! / compute_product_of_messages! /
 *                          compute_joint_marginal!                         src/inference_engine.jl:351-477
 *   cx_sweep             update_marginals!(engine, variable_ids)           src/inference_engine.jl:559-632
 *                        (device "flooding" schedule over the whole graph)
 *   cx_get_marginals     get_value(get_variable_marginal(variable))        src/model_engine.jl:60-62
 *   cx_get_messages      get_value(message_to_variable / message_to_factor) src/model_engine.jl:207-222
 *
 * Conventions
 *   - plain C: pointers + sizes, no C++/torch types; every function returns an int32 status
 *     (CX_OK == 0, negative = error) and never throws or longjmps across the boundary;
 *     cx_last_error() returns the text a Julia shim passes to error().
 *   - ids are the reference's ids: 1-based Int64, one id space shared by variables and factors
 *     (BipartiteFactorGraphs add_variable!/add_factor!).  Neighbour order is ascending id.
 *   - Gaussian payloads cross the boundary in MOMENT form like the reference's test structs
 *     (test/runtests.jl:31-34 NormalMeanVariance): dim==1: {mean, variance};
 *     dim==d: mean[d] then covariance[d*d] row-major.  NaN variance/covariance == UndefValue().
 *   - the caller owns every pointer it passes; the library copies before returning and owns all
 *     device memory behind the opaque handle.  One caller thread per handle.
 *   - calls are asynchronous on the handle's HIP stream unless they return data to the host;
 *     cx_sync() waits.
 */
#ifndef CORTEX_HIP_H
#define CORTEX_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CX_ABI_VERSION 9   /* 9: cx_linear_moments (additive).  8: cx_predictive, cx_predictive_rows (additive).  7: cx_sample_posterior (additive).  6: cx_factor_beliefs, cx_factor_statistics (additive).  5: cx_log_evidence (additive).  4: cx_config.sweeps_per_launch -> reserved, cx_tile_stats and CX_KERNEL_TILED removed.  3: CX_SCHED_REFERENCE, cx_sweep_for, cx_ref_plan_stats, cx_ref_trace, cx_set_damping.  2: cx_config.reserved became sweeps_per_launch (validated), five new item / factor kinds, state blobs "CXSTATE2" */

/* status codes */
#define CX_OK 0
#define CX_ERR_INVALID_ARGUMENT (-1)  /* bad pointer / size / enum */
#define CX_ERR_NOT_FOUND (-2)         /* unknown variable / factor / edge id */
#define CX_ERR_UNSUPPORTED (-3)       /* factor arity / kind / dim the device path does not implement */
#define CX_ERR_STATE (-4)             /* call order (e.g. sweep before graph) */
#define CX_ERR_DEVICE (-5)            /* HIP runtime error; text in cx_last_error */
#define CX_ERR_NO_DEVICE (-6)         /* no gfx950 device visible */
#define CX_ERR_OUT_OF_MEMORY (-7)

/* message direction: which of a Connection's two signals (model_engine.jl:181-186) */
#define CX_TO_FACTOR 1    /* MessageToFactor(variable_id, factor_id),   inference_signal.jl:29-32 */
#define CX_TO_VARIABLE 2  /* MessageToVariable(variable_id, factor_id), inference_signal.jl:45-48 */

/* work-item kinds of cx_update_batch == the variants process! dispatches on */
#define CX_ITEM_MESSAGE_TO_FACTOR 1
#define CX_ITEM_MESSAGE_TO_VARIABLE 2
#define CX_ITEM_INDIVIDUAL_MARGINAL 4
#define CX_ITEM_PRODUCT_OF_MESSAGES 8  /* ProductOfMessages(variable_id, range, factors), inference_signal.jl:62-66: the product of
                                          the factor→variable messages number lo..hi (1-based, inclusive, ascending factor id:
                                          the reference's `range` over factors_connected_to_variable) of variable_id — the
                                          segment-tree intermediates of dependencies.jl:128-173.  ORDERING ASSUMPTION: the range is
                                          resolved over the variable's factors in ascending id order; a plug-in whose model engine
                                          lists factors_connected_to_variable in another order must refuse or translate (the Python
                                          and Julia plug-ins check it).  The range travels in
                                          cx_item.factor_id as CX_ITEM_RANGE(lo, hi); the value is kept in a device store
                                          (cx_get_products) */
#define CX_ITEM_JOINT_MARGINAL 16      /* JointMarginal(factor_id, variable_ids), inference_signal.jl:93-96, for a pairwise
                                          Gaussian factor: the 2-d Gaussian ∝ factor x the two variable→factor messages
                                          (compute_joint_marginal!, inference_engine.jl:469-477); variable_id is ignored, the
                                          value is kept in a device store (cx_get_joint_marginals) */
#define CX_ITEM_RANGE(lo, hi) ((int64_t)(((uint64_t)(uint32_t)(lo) << 32) | (uint64_t)(uint32_t)(hi)))

/* payload forms */
#define CX_FORM_MOMENT 0  /* Gaussian (mean, variance|covariance) */
#define CX_FORM_POINT 1   /* observed datum: the `Real` input of test/inference_engine_tests.jl:424 ; dim values */
#define CX_FORM_NATURAL 2 /* (xi = precision*mean, w = precision): the library's storage form */
#define CX_FORM_MEAN_PRECISION 3 /* NormalMeanPrecision(mean, precision), test/runtests.jl:48-56 (variational families) */
#define CX_FORM_GAMMA 4          /* Gamma(shape, scale), test/runtests.jl:60-67 (variational families) */

/* factor kinds (what the user rule reads from Factor.functional_form, model_engine.jl:119-122) */
#define CX_FACTOR_OPAQUE 0          /* messages only ever set by the caller (priors, unary observations) */
#define CX_FACTOR_GAUSS_ADDITIVE 1  /* 2 edges: x_b = x_a + N(0, q)            params = {q}                */
#define CX_FACTOR_GAUSS_LINEAR 2    /* 2 edges: x_out = a*x_in + b + N(0, q)   params = {q, a, b}          */
                                    /* dim>1:   x_out = A x_in + b + N(0, Q)   (A, Q) via cx_set_factor_matrices; b per factor, 0 unless set
                                                                               by cx_set_factor_offsets (dim 2 - 4) */
#define CX_FACTOR_NORMAL_PRECISION 3 /* 3 edges: x_out ~ N(x_in, 1 / precision); roles OUT, IN, PRECISION — the :likelihood and
                                       :transition factors of test/inference_engine_tests.jl:691-715.  Variational rules only: the
                                       CX_FAMILY_VMP_* families, or CX_FAMILY_GAUSSIAN under CX_SCHED_REFERENCE with a user wiring
                                       (cx_graph_wire, ABI 3) */
#define CX_FACTOR_BERNOULLI 4        /* CX_FAMILY_NATURAL2, 2 edges: one variable carries an observed Bool r (a CX_FORM_POINT datum),
                                       the message to the other is Beta(1 + r, 2 - r) = natural (r, 1 - r): the :bernoulli
                                       factor of test/inference_engine_tests.jl:250-262.  Without a datum the reference's rule
                                       is error(...): the message stays undefined */
#define CX_FACTOR_GAUSS_LINEAR_N 5   /* 3 to 7 edges.  dim 2, 3, 4 (ABI 3): x_out = A_1 x_1 + ... + A_k x_k + N(0, Q), params = {parameter set}: its Q is the noise, its A
                                        every input's matrix unless cx_set_factor_edge_sets names another set for an edge; fused and tree schedules,
                                        batch items.  dim == 1: x_out = a_1 x_1 + ... + a_k x_k + b + N(0, q), k = 2..6 inputs; params = {q, b};
                                        exactly one CX_ROLE_OUT edge, the others CX_ROLE_IN; a_i = 1 unless cx_set_factor_coefficients says
                                        otherwise.  Every factor→variable message of the factor reads ALL its other variable→factor
                                        messages (src/dependencies.jl:17-31).  Flooding, fused, tree and reference-order schedules; under partitions
                                        with state halos (cx_halo_configure_state), not with per-sweep message halos. */
#define CX_NPARAM 4                 /* doubles per factor in factor_params */

/* edge roles for directed factors (Connection.label :out/:in, model_engine.jl:182) */
#define CX_ROLE_OUT 0
#define CX_ROLE_IN 1
#define CX_ROLE_PRECISION 2   /* the Gamma-distributed precision of a CX_FACTOR_NORMAL_PRECISION factor */

/* message families for dim == 1.  The sweep's products are sums of natural parameters for ANY exponential family; only
 * the factor rules, the moment conversions at the ABI and the marginal read-out are Gaussian-specific. */
#define CX_FAMILY_GAUSSIAN 0  /* (xi, w); marginals and MOMENT payloads are (mean, variance) */
#define CX_FAMILY_NATURAL2 1  /* any 2-parameter family in natural coordinates, e.g. Beta(a, b) as (a-1, b-1): the
                                 Beta-Bernoulli model of test/inference_engine_tests.jl:241-377.  Payloads are NATURAL (data:
                                 POINT), factors are CX_FACTOR_OPAQUE (their messages are set by the caller) or
                                 CX_FACTOR_BERNOULLI, marginals come back as the natural-parameter sums. */
/* Variational message passing: messages depend WEAKLY on marginals (add_dependency!(...; weak = true), signal.jl:36-45).
 * The state is the set of marginals (cx_set_marginals / cx_update_marginals / cx_get_marginals); cx_sweep, cx_update_batch
 * and the message accessors do not apply.  Factors are CX_FACTOR_NORMAL_PRECISION, dim == 1. */
#define CX_FAMILY_VMP_MEAN_FIELD 2  /* fully factorised posterior: the MeanFieldResolver + SSMMeanFieldInferenceRequestProcessor
                                       of test/inference_engine_tests.jl:599-689 */
#define CX_FAMILY_VMP_STRUCTURED 3  /* Normal variables jointly (belief propagation with E[precision], run with cfg.schedule —
                                       CX_SCHED_CHAIN_SCAN gives the exact forward/backward pass per update, CX_SCHED_TREE the exact
                                       two passes when the states form any forest), precisions from the joint marginals:
                                       StructuredResolver + SSMStructuredInferenceRequestProcessor, :810-1030 */

/* schedules of cx_sweep */
#define CX_SCHED_FLOODING 0   /* all variable→factor, then all factor→variable, then marginals           */
#define CX_SCHED_FUSED 1      /* same fixed-point map, one fused kernel on double-buffered messages        */
#define CX_SCHED_CHAIN_SCAN 2 /* graphs whose non-observed variables form disjoint chains (state-space models):
                                 one cx_sweep = the exact forward/backward result of the reference's sequential
                                 schedule (inference_engine.jl:575-608), by two parallel prefix scans.  When every
                                 non-observed variable is on a chain and materialize_messages_to_factor is 0, the
                                 scan writes the marginals itself and variable→factor messages are recomputed from
                                 the stored messages when cx_get_messages / cx_update_batch ask for them.
                                 dim 1, 2, 3, 4.  For dim 2..4 (scan over composed linear-Gaussian maps) every
                                 non-observed variable must sit on a chain; a sweep writes the marginals, the chain
                                 messages reach their slots when cx_get_messages / cx_update_batch / cx_residual /
                                 cx_state_export ask for them                                                     */
#define CX_SCHED_TREE 3       /* graphs whose non-observed part is a forest (any degrees, factors of two or more variables):
                                 one cx_sweep = the reference's one update_marginals! there — every message once, from
                                 final inputs, leaves to root and back (inference_engine.jl:575-608), level by level:
                                 2 x depth + 1 launches over item lists built once (depth = half the longest path of a
                                 component, counted in variables and factors).  A cycle among the non-observed variables
                                 is refused (CX_ERR_UNSUPPORTED).  Lazy like the reference: nothing into observed
                                 variables.  dim 1 (Gaussian and natural-pair families), 2, 3, 4 and 64 (5 .. 63 with it).  */
#define CX_SCHED_REFERENCE 4  /* ANY graph, loops included: one cx_sweep / cx_sweep_for = the reference's one update_marginals! —
                                 the same signals computed in the same ORDER, each from exactly the values the reference's rule call
                                 read (a sequential pass that always reads the newest values, inference_engine.jl:575-608,
                                 signal.jl:466-490: "Gauss-Seidel" in requested-variable order x neighbour order).  The library keeps a
                                 shadow of every signal's readiness nibbles, wired as DefaultDependencyResolver wires them
                                 (dependencies.jl:17-173, signal.jl:141-154,232-253,668-730) and driven by cx_set_messages /
                                 cx_seed_messages (the user's set_value!), cx_update_batch (a plug-in's process!) and the sweeps; a call
                                 runs the reference's scheduler on the shadow, records the executions, levels them (an execution's stage
                                 follows every execution whose result it reads, every reader of the value it overwrites, and its own
                                 previous one) and replays the stages as item lists in ONE launch: an XCD-resident cluster — the
                                 workgroups of one XCD behind barriers that stay in that XCD's L2 — for plans of wide stages (such a call
                                 returns when it has finished: the host checks that no barrier timed out), a HIP graph of stage launches
                                 for chains of thin ones (asynchronous).  Plans are kept per (readiness
                                 state at the start of the call, request): the steady state of "set the priors, call" replays a standing
                                 plan.  Lazy like the reference: a call computes what is pending for the requested marginals, nothing
                                 else; priors have to be re-set before a call to be fresh, exactly as there.  On a forest it is the tree
                                 schedule with requests for some of the variables.  dim 2, 3, 4 (ABI 3): linear-Gaussian factors of two to seven
                                 variables, variables of any degree, the default wiring (the stages run through the batched d-dimensional items;
                                 variable→factor messages are stored signals there, not recomputed for a reader).  dim 1 (Gaussian and natural-pair families), factors
                                 of any arity the rules have, variables of any degree (degree > 5: the segment-tree nodes of
                                 dependencies.jl:90-173 are computed, stored and read one by one, as the reference does).  Not partitioned. */


typedef struct cx_handle cx_handle;

typedef struct cx_config {
    int32_t struct_size;   /* sizeof(cx_config), for forward compatibility */
    int32_t device;        /* HIP device ordinal */
    int32_t dim;           /* message dimension d: 1 (scalar), 2, 3, 4 (registers); 5 .. 64 run on the f64 matrix cores, a wave per message, in
                              1 x 1, 2 x 2 or 4 x 4 accumulator tiles of 16: the smallest of 16, 32, 64 that holds d, under every schedule
                              (ABI 4; cx_chain_block_maps: dim 1 .. 4 and 64 only).  A d in between is embedded
                              block-diagonally (x, u) with u a unit random walk nobody observes: exact results for the d x d blocks,
                              payloads of d and d + d*d doubles as for any d, at the cost of the tile size                          */
    int32_t schedule;      /* CX_SCHED_*: dim 1 all five; dim 2 .. 64: CX_SCHED_FUSED, CX_SCHED_CHAIN_SCAN, CX_SCHED_TREE, CX_SCHED_REFERENCE */
    int32_t compute_marginals_in_sweep; /* 1: every sweep also refreshes all marginals (update_marginals!); after cx_sweep(h, n) they are
                                           those of its LAST sweep — under the fused and flooding schedules without a halo the earlier
                                           sweeps of one call, whose marginals nobody can read, do not store them.
                                           2 (CX_SCHED_CHAIN_SCAN, dim 2..4; elsewhere the same as 1): on demand — a sweep leaves
                                           the chain's forward and backward sums in the order of its walks, and the pass that
                                           adds them up, converts to moment form and moves them to the marginals' place runs
                                           before the first cx_state_export / cx_update_batch / cx_get_marginals of an eighth of
                                           the variables or more after it; a cx_get_marginals for fewer forms just those
                                           (the same values; dim 64 always works this way)                                  */
    int32_t materialize_messages_to_factor; /* CX_SCHED_FUSED only. 0: variable→factor messages stay in registers
                                               during a sweep and are recomputed, bit-identically, from the retained
                                               input buffer when cx_get_messages / cx_update_batch asks for them;
                                               1: every sweep also stores them */
    int32_t family;        /* CX_FAMILY_*: what a scalar (dim == 1) message's two numbers mean */
    int32_t reserved;      /* 0 (1 is accepted).  ABI 2 - 3: sweeps_per_launch — the two-sweeps-per-launch kernel (temporal blocking in
                              LDS; bit-identical, measured 1.8 - 2x slower than two single sweeps, HISTORY.md) was removed in ABI 4 */
} cx_config;

typedef struct cx_item {
    int32_t kind;          /* CX_ITEM_* */
    int32_t reserved;
    int64_t variable_id;
    int64_t factor_id;     /* ignored for CX_ITEM_INDIVIDUAL_MARGINAL; CX_ITEM_RANGE(lo, hi) for CX_ITEM_PRODUCT_OF_MESSAGES */
} cx_item;

typedef struct cx_stats {
    int64_t n_variables, n_factors, n_edges;
    int64_t n_messages_per_sweep;     /* directed messages with >=1 dependency and >=1 listener: the metric's unit */
    int64_t n_slices, n_big_variables, n_slots; /* SELL-256 slices, CSR-tail variables, message slots incl. padding */
    int64_t device_bytes;
    int64_t sweeps_done;
} cx_stats;

/* ---- lifecycle ---------------------------------------------------------------------------- */
int32_t cx_version(void);
int32_t cx_create(const cx_config *config, cx_handle **out);
int32_t cx_destroy(cx_handle *h);                 /* idempotent on NULL */
const char *cx_last_error(const cx_handle *h);    /* h may be NULL: last error of a failed cx_create */
int32_t cx_sync(cx_handle *h);
int32_t cx_set_stream(cx_handle *h, void *hip_stream); /* run on the caller's hipStream_t (NULL = default) */

/* ---- graph ingestion: BipartiteFactorGraph{Variable,Factor,Connection} flattened once --------
 * edge_var[e], edge_fac[e]: the (variable_id, factor_id) of every Connection, any order.
 * factor_ids[f], factor_kind[f], factor_params[f*CX_NPARAM ..]: one row per factor.
 * edge_role may be NULL (all CX_ROLE_OUT); it is only read for CX_FACTOR_GAUSS_LINEAR.
 * Replaces get_variable_ids/get_factor_ids/get_connected_*_ids/get_connection
 * (model_engine.jl:329-391) and fixes the dependency wiring of DefaultDependencyResolver
 * (dependencies.jl:17-126) into gather lists. */
int32_t cx_graph_create(cx_handle *h, int64_t n_edges, const int64_t *edge_var, const int64_t *edge_fac,
                        const int32_t *edge_role, int64_t n_factors, const int64_t *factor_ids,
                        const int32_t *factor_kind, const double *factor_params);
/* dim > 1: parameter set `parameter_set` of the linear-Gaussian factors x_out = A x_in + b + N(0, Q); A, Q are d x d row-major,
 * Q symmetric positive definite; b is the factor's own (cx_set_factor_offsets, dim 2 - 4; 0 otherwise).  A CX_FACTOR_GAUSS_LINEAR factor names its set in factor_params[0]; its ROLE_IN edge carries
 * x_in.  (The reference leaves Factor.functional_form opaque, model_engine.jl:119-122; this is what the user rule reads.) */
int32_t cx_set_factor_matrices(cx_handle *h, int64_t parameter_set, const double *A, const double *Q);
/* a_i of ROLE_IN edges of CX_FACTOR_GAUSS_LINEAR_N factors (finite, non-zero; default 1).  Takes effect at the next sweep. */
int32_t cx_set_factor_coefficients(cx_handle *h, int64_t n, const int64_t *variable_ids, const int64_t *factor_ids, const double *a);
/* dim 2, 3, 4: x_out = A_1 x_1 + ... + A_k x_k + N(0, Q) for a CX_FACTOR_GAUSS_LINEAR_N factor: the factor's params[0] names the parameter set
 * whose Q is the noise and whose A is every input's matrix; this call gives the CX_ROLE_IN edge (variable, factor) the A of another set. */
int32_t cx_set_factor_edge_sets(cx_handle *h, int64_t n, const int64_t *variable_ids, const int64_t *factor_ids, const int64_t *parameter_sets);
int32_t cx_graph_stats(const cx_handle *h, cx_stats *out);
/* position of Connection (variable_id, factor_id) in the flattened edge table (sorted by variable, factor) */
int32_t cx_edge_index(const cx_handle *h, int64_t n, const int64_t *variable_ids, const int64_t *factor_ids,
                      int64_t *out_edge);

/* ---- data injection / read-back --------------------------------------------------------------
 * payload: n rows of cx_payload_doubles(dim, form) doubles.
 * The variable→factor message of a non-observed variable of degree 1 (the last state of a forecast, a latent leaf) is the caller's:
 * CX_FORM_NATURAL zeros is the flat message, which leaves the rest of the model as it is; left unset, it leaves the marginals of
 * every other variable of its component undefined. */
int64_t cx_payload_doubles(int32_t dim, int32_t form);
int32_t cx_set_messages(cx_handle *h, int64_t n, const int64_t *variable_ids, const int64_t *factor_ids,
                        int32_t direction, int32_t form, const double *payload);
int32_t cx_get_messages(cx_handle *h, int64_t n, const int64_t *variable_ids, const int64_t *factor_ids,
                        int32_t direction, int32_t form, double *out);
/* ---- variational families: the marginals are the state -------------------------------------------------------------
 * cx_set_marginals    : the user's set_value!(get_variable_marginal(...), value) (test/inference_engine_tests.jl:717-727,
 *                       :734-736): CX_FORM_POINT observes a Normal variable (1 double), CX_FORM_MEAN_PRECISION /
 *                       CX_FORM_MOMENT initialise a latent Normal variable, CX_FORM_GAMMA a precision variable (2 doubles).
 * cx_update_marginals : one update_marginals!(engine, variable_ids) (src/inference_engine.jl:559-632) under the weak
 *                       wiring: the messages into the requested variables are computed from the marginals as they stand
 *                       before the call, then the requested marginals are stored.  n may be CX_VMP_ALL_NORMAL or
 *                       CX_VMP_ALL_PRECISION (variable_ids ignored) to name a whole class without an id list.
 *                       CX_FAMILY_VMP_STRUCTURED updates the latent Normal variables together.  A request that names them TOGETHER
 *                       with precision variables (the last call of the reference's experiment, test/inference_engine_tests.jl:1113)
 *                       is evaluated by the reference in an order that emerges from its lazy readiness flags; it is accepted where
 *                       that order is class by class — transition precisions, states, other precisions — i.e. when the states were
 *                       updated before, every precision of a transition factor (degree > 5) precedes the first state in the list and
 *                       every other requested precision was updated since the states last were; CX_ERR_UNSUPPORTED otherwise (the
 *                       reference then interleaves per variable).  Asynchronous on the handle's stream.
 * cx_get_marginals    : (mean, precision) for Normal variables ((datum, +inf) when observed), (shape, scale) for precisions.
 * cx_set_marginals also serves CX_SCHED_REFERENCE handles (dim 1) whose wiring makes messages depend on marginals (cx_graph_wire): the
 * same forms; there cx_get_marginals returns (mean, variance) for Normal variables — the Gaussian family's form — and (shape, scale) for
 * precisions. */
#define CX_VMP_ALL_NORMAL (-1)
#define CX_VMP_ALL_PRECISION (-2)
int32_t cx_set_marginals(cx_handle *h, int64_t n, const int64_t *variable_ids, int32_t form, const double *payload);
int32_t cx_update_marginals(cx_handle *h, int64_t n, const int64_t *variable_ids);

/* give every still-undefined message of `direction` the value N(mean, variance*I): the seeding a user of
 * the reference does by hand before loopy BP (cf. test/inference_engine_tests.jl:729-736) */
int32_t cx_seed_messages(cx_handle *h, int32_t direction, double mean, double variance);
int32_t cx_get_marginals(cx_handle *h, int64_t n, const int64_t *variable_ids, double *out);

/* ---- compute ---------------------------------------------------------------------------------- */
/* one launch for a batch of mutually independent signals, in the caller's order of enqueue.  dim == 1: all five item kinds;
 * dim 2, 3, 4, 64: CX_ITEM_MESSAGE_TO_FACTOR, CX_ITEM_MESSAGE_TO_VARIABLE, CX_ITEM_INDIVIDUAL_MARGINAL (for dim 64 a marginal is
 * computed from the stored messages when cx_get_marginals reads it: the item only checks its variable).  A result with an undefined
 * dependency is not stored (the signal was not pending, src/signal.jl:668-730).
 * cx_update_batch is complete at return.  cx_update_batch_async is the same call without the wait for batches of up to 48 items
 * (dim 1 - 4): their records travel in the kernel arguments and the call returns when the launch is queued, like cx_sweep — what
 * a scheduler does next (set_value!, readiness bits: signal.jl:232-253) does not read the device, and every cx_get_* /
 * cx_residual / cx_sync waits for the stream.  Larger batches and dim 64 stage their records through a buffer of the handle and
 * are complete at return in both forms. */
int32_t cx_update_batch(cx_handle *h, const cx_item *items, int64_t n);
int32_t cx_update_batch_async(cx_handle *h, const cx_item *items, int64_t n);
/* values of the intermediates cx_update_batch keeps on the device: ProductOfMessages nodes (2 doubles each — dim > 1: a message
 * payload of d + d * d doubles each; the reference's default resolver creates them for variables of degree > 5; any degree — `form` CX_FORM_MOMENT or CX_FORM_NATURAL) and JointMarginal nodes (dim 1) (6 doubles each: mean[2], covariance[4] row-major, variables in
 * ascending id order).  A node never computed reads as NaN (UndefValue()). */
int32_t cx_get_products(cx_handle *h, int64_t n, const int64_t *variable_ids, const int32_t *range_lo, const int32_t *range_hi,
                        int32_t form, double *out);
int32_t cx_get_joint_marginals(cx_handle *h, int64_t n, const int64_t *factor_ids, double *out);
/* n_sweeps passes of the configured device schedule over the whole graph (asynchronous) */
int32_t cx_sweep(cx_handle *h, int32_t n_sweeps);
/* Damping for the schedules that iterate to a fixed point (CX_SCHED_FUSED, CX_SCHED_FLOODING; dim 1 - 4): every factor→variable message a
 * sweep computes is stored as (1 - lambda) x rule + lambda x the message it replaces, in natural parameters (an undefined old message does
 * not damp).  0 <= lambda < 1, 0 (the default) = off: the sweeps are then bit for bit what they were.  The fixed point is unchanged; loopy
 * Gaussian BP that oscillates outside the walk-summable regime converges under enough damping.  The reference has no counterpart: its rules
 * are the user's code, a user damps inside them.  Not with per-sweep message halos (cx_halo_configure); state halos are damped like the
 * plain sweeps they run. */
int32_t cx_set_damping(cx_handle *h, double lambda);
/* CX_SCHED_REFERENCE: ONE update_marginals!(engine, variable_ids) (src/inference_engine.jl:559-632; request_inference_for :298-323) for
 * the named variables in the caller's order — only what is pending for those marginals is computed (cx_sweep requests every variable
 * that is neither observed nor a stand-in, in ascending id order).  Other schedules: CX_ERR_UNSUPPORTED (they compute every message). */
int32_t cx_sweep_for(cx_handle *h, int64_t n, const int64_t *variable_ids);
/* CX_SCHED_REFERENCE: a user resolver's dependency wiring in place of DefaultDependencyResolver's (src/dependencies.jl:1-15): the i-th triple is
 * add_dependency!(signals[i], dependencies[i]; weak, intermediate, listen) (src/signal.jl:286-337), in call order (= dependency order per
 * signal).  Signals are named like batch items: CX_ITEM_MESSAGE_TO_FACTOR / CX_ITEM_MESSAGE_TO_VARIABLE (variable_id, factor_id),
 * CX_ITEM_INDIVIDUAL_MARGINAL (variable_id), CX_ITEM_JOINT_MARGINAL (factor_id).  The scheduler runs on whatever is wired; the VALUES come
 * from the device's rules, so a dependency list must be one a rule can serve:
 *   - a MessageToFactor / IndividualMarginal depends on MessageToVariable signals of its own variable: its value is the product of exactly
 *     its dependency list, in list order (a dropped dependency is left out of the product);
 *   - a MessageToVariable of a sum-product factor (additive, linear, linear-N) depends on MessageToFactor signals of its factor's other
 *     variables: its value is the factor's rule on the stored messages of the factor's other edges;
 *   - the messages of a CX_FACTOR_NORMAL_PRECISION factor (out ~ N(in, 1 / precision), precision Gamma-distributed) depend on MARGINALS — the
 *     variational rules of the reference's test processors (test/inference_engine_tests.jl:647-689, 939-1030), chosen by the dependency list as
 *     those rules choose:   to out / in     <- marginal(in / out), marginal(precision)              N(E[other], E[precision])
 *                           to precision    <- marginal(out), marginal(in)                          Gamma(3/2, 2 / (var out + var in + (E out - E in)^2))
 *                           to out / in     <- MessageToFactor(in / out), marginal(precision)       N(mean m, 1 / (var m + 1 / E[precision]))
 *                           JointMarginal   <- MessageToFactor(out), MessageToFactor(in), marginal(precision)    the 2-d Gaussian of :939-967
 *                           to precision    <- JointMarginal(factor)                                Gamma(3/2, 2 / (V11 - 2 V12 + V22 + (m1 - m2)^2))
 *     Such factors exist under this schedule only.  A variable on a CX_ROLE_PRECISION edge is Gamma-distributed everywhere: its messages are the
 *     natural pairs (shape - 1, rate) (CX_FORM_NATURAL; a prior is an opaque factor's message), its marginal is kept and returned as
 *     (shape, scale); Normal variables as (mean, variance).  Initial marginals and data: cx_set_marginals (CX_FORM_GAMMA; CX_FORM_MOMENT /
 *     CX_FORM_MEAN_PRECISION; CX_FORM_POINT = an observed value, variance 0), the user's set_value! on the marginal signal.
 * Anything else is CX_ERR_UNSUPPORTED, as are intermediate flags that close a cycle (process_dependencies! would never return) and a
 * dependency listed twice.  Two flags stand for calls other than add_dependency!:
 *   CX_WIRE_DEFAULT_VARIABLE  signals[i] = IndividualMarginal(v), dependencies[i] ignored: resolve_variable_dependencies!(
 *                             DefaultDependencyResolver(), engine, v) at this point of the call order (src/dependencies.jl:33-126: all-pairs up to
 *                             degree 5, a segment tree of ProductOfMessages above; a MessageToFactor is wired only if something listens to it by now)
 *   CX_WIRE_LINK              signals[i] = JointMarginal(f), dependencies[i] = IndividualMarginal(v): link_signal_to_variable!(v, signal)
 *                             (src/model_engine.jl:64-71): requested and computed with v's marginal (src/inference_engine.jl:313-315, 617-625)
 * Replaces the whole wiring (n == 0: none); allowed until the first value is set or the first call runs, as the reference wires at engine
 * construction.  The two fused families (cx_update_marginals) remain the fast path for the reference's two test models; this entry point runs
 * them, and any other wiring of these rules on any graph, call by call as the reference's scheduler would — mixed requests included.
 * dim 1: all of the above.  dim 2, 3, 4 (ABI 4): wirings of the sum-product rules (a MessageToFactor / marginal is the sum of ITS dependency
 * list); dim 64 forms marginals from all stored messages when they are read and refuses wirings. */
#define CX_WIRE_WEAK 1          /* add_dependency!(...; weak = true): the dependency need only be computed, not fresh (src/signal.jl:36-45) */
#define CX_WIRE_INTERMEDIATE 2  /* intermediate = true: process_dependencies! descends through it (src/signal.jl:466-490) */
#define CX_WIRE_NO_LISTEN 4     /* listen = false: the dependency's set_value! does not make the signal potentially pending */
#define CX_WIRE_DEFAULT_VARIABLE 8
#define CX_WIRE_LINK 16
int32_t cx_graph_wire(cx_handle *h, int64_t n, const cx_item *signals, const cx_item *dependencies, const int32_t *flags);
/* the plan the last reference-order call replayed: out8 = { stages, kernel launches, executions (signals computed), of which messages,
 * passes of the reference's loop (the final marginal round included), plans kept, calls that replayed a kept plan, calls that had to
 * run the scheduler }.  Zeros before the first call and for other schedules. */
int32_t cx_ref_plan_stats(const cx_handle *h, int64_t *out8);
/* the scalar chain scan as ONE launch (CX_SCHED_CHAIN_SCAN, the scans of CX_SCHED_TREE's heavy paths, the variational families' state
 * pass): a single-pass scan whose workgroups publish their tile totals under the launch's tag instead of ending a kernel
 * (csrc/cx_chain.hip: k_chain_onepass).  Taken when the whole grid is resident at once (up to twice the compute units' count of tiles); every wait is bounded in time (0.5 s, CX_CHAIN_ONEPASS_TIMEOUT_MS) —
 * a launch whose wait times out stores NOTHING, the next call that checks the device returns CX_ERR_DEVICE, the handle goes back to the
 * two-launch scan and the caller repeats the sweep (a chain-scan sweep is exact whatever it starts from).  CX_CHAIN_ONEPASS=0 turns it off.
 * out4 = { 1 ready / 0 not prepared / -1 off, launches of the one-launch form so far, G, 0 } — G counts another kind of fused launch: the
 * sweeps between two exchanges of a deep-halo partition (cx_halo_configure_state + cx_halo_set_layers) replayed as ONE graph launch once
 * the same batch has been asked for twice — with CX_HALO_GRAPH=1 only: measured 2 - 5 % slower than the plain launches on MI355X, off by default. */
int32_t cx_chain_scan_stats(const cx_handle *h, int64_t *out4);
/* diagnostics of the fused sweep (additive, still ABI 8; tests): out4[0] entries of the partner-run table (four per 256-slot row; 0: the
 * graph's partners do not fit 16-bit differences, no table), [1] those that fall back to the per-lane index, [2] sweeps of cx_sweep
 * calls so far that stored no marginals (every sweep of a call but the last), [3] launches so far that ran two sweeps at once (grids:
 * floor((n - 1) / 2) per cx_sweep(h, n) call; CX_SWEEP_PAIRS=0 in the environment turns them off) */
int32_t cx_sweep_stats(const cx_handle *h, int64_t *out4);
/* ... and of its deep launches (additive; tests): in a cx_sweep call of at least 16 sweeps the sweeps before the last run three to six to
 * a launch (CX_SWEEP_DEPTH=2 .. 6 forces the depth, CX_DEEP_ROWS the rows per segment; CX_SWEEP_PAIRS=0 turns every multi-sweep launch
 * off).  out4 = { launches so far at depth 3, at depth 4, the depth of the last call that ran multi-sweep launches (2 in a call of fewer
 * than 16 sweeps; 0: none yet, or no grid plan), the rows per segment at that depth }.  cx_sweep_stats' [3] keeps counting depth 2 only. */
int32_t cx_sweep_deep_stats(const cx_handle *h, int64_t *out4);
/* ... by depth (additive; tests): out7[d] = launches so far that ran d sweeps at once, d = 2 .. 6 (CX_SWEEP_DEPTH=2 .. 6; [2] is
 * cx_sweep_stats' [3]); out7[0] = out7[1] = 0 */
int32_t cx_sweep_deep_launches(const cx_handle *h, int64_t *out7);
/* the XCD-resident cluster (reference-order plans of many dependent stages of 1 - 16 k items — calls on loopy graphs — run as ONE launch
 * of the workgroups of one XCD behind barriers that stay in that XCD's L2): out4 = { 1 ready / 0 not prepared / -1 off
 * (CX_REF_CLUSTER=0, a device that is neither gfx942 nor gfx950, or a barrier once timed out), workgroups per launch (compute units),
 * calls RECOVERED (every wait of the cluster is bounded in time — 1.5 s, CX_REF_CLUSTER_TIMEOUT_MS; a call whose cluster gives up is
 * finished from its first incomplete stage on plain launches, returns CX_OK with the same results, and the handle stays with launches),
 * 1 when the last reference-order call ran on the cluster }. */
int32_t cx_cluster_stats(const cx_handle *h, int64_t *out4);
/* the executions of the last reference-order call in the reference's order — what a `trace = true` engine records
 * (src/inference_engine.jl:650-862: TracedInferenceExecution.signal), as items (kind, variable_id, factor_id | CX_ITEM_RANGE).
 * *n_executions = their number; out (may be NULL) receives the first `capacity` of them. */
int32_t cx_ref_trace(const cx_handle *h, int64_t capacity, cx_item *out, int64_t *n_executions);
/* max over directed messages of |Δmean|, |Δvariance| between the last two sweeps (host-synchronous) */
int32_t cx_residual(cx_handle *h, double *out_max_abs_delta);
/* sweep until cx_residual over `check_every` sweeps is <= tol, or max_sweeps have run (stopping rule for loopy graphs; the
 * reference leaves it to the caller of update_marginals!).  A NaN residual (undefined messages) never satisfies tol. */
int32_t cx_sweep_until(cx_handle *h, double tol, int32_t max_sweeps, int32_t check_every, int32_t *sweeps_run, double *residual);

/* ---- partitioned graphs (one handle per GPU; exchange is the caller's: RCCL/torch.distributed) --
 * Cut edges appear in this rank's graph as degree-1 "ghost" variables whose variable→factor message is
 * produced by another rank.  cx_halo_configure names the edges this rank exports / imports; buffers hold
 * NATURAL-form payloads (2 doubles per edge for dim == 1), in list order. */
int32_t cx_halo_configure(cx_handle *h, int64_t n_send, const int64_t *send_variable_ids,
                          const int64_t *send_factor_ids, int64_t n_recv, const int64_t *recv_variable_ids,
                          const int64_t *recv_factor_ids);
int32_t cx_halo_buffers(cx_handle *h, void **send_device_ptr, int64_t *send_bytes, void **recv_device_ptr,
                        int64_t *recv_bytes);
/* use caller-owned device buffers (e.g. torch tensors handed to torch.distributed) instead of the library's */
int32_t cx_halo_set_buffers(cx_handle *h, void *send_device_ptr, void *recv_device_ptr);
/* one partitioned sweep = three asynchronous calls, so the caller can overlap the exchange with the main kernel:
 *   cx_sweep_begin : compute the exported variable→factor messages and pack them into the send buffer
 *   [caller starts the exchange of send → peer's recv buffer on its communication stream]
 *   cx_sweep_main  : the sweep over every variable this rank owns
 *   [caller makes the handle's stream wait for the exchange]
 *   cx_sweep_end   : unpack the recv buffer into the ghost variables and push it through the cut factors
 * The three calls together compute exactly one cx_sweep of the un-partitioned graph. */
int32_t cx_sweep_begin(cx_handle *h);
int32_t cx_sweep_main(cx_handle *h);
int32_t cx_sweep_end(cx_handle *h);

/* The same three steps with the exchange issued by the library itself on RCCL (grouped ncclSend/ncclRecv with the
 * partition neighbours on a dedicated stream, overlapped with the main kernel) — no host language in the per-sweep loop.
 *   cx_comm_unique_id : rank 0 obtains the 128-byte ncclUniqueId and distributes it by any means
 *   cx_comm_init      : every rank joins (one communicator per handle)
 *   cx_halo_peers     : which segments (in messages) of the send / recv lists of cx_halo_configure belong to which rank
 *   cx_sweep_exchange : n_sweeps x { begin, exchange, main, end }, asynchronous on the handle's stream */
int32_t cx_comm_unique_id(void *out128);
int32_t cx_comm_init(cx_handle *h, int32_t world, int32_t rank, const void *id128);
int32_t cx_halo_peers(cx_handle *h, int32_t n_peers, const int32_t *peer_rank, const int64_t *send_offset,
                      const int64_t *send_count, const int64_t *recv_offset, const int64_t *recv_count);
int32_t cx_sweep_exchange(cx_handle *h, int32_t n_sweeps);

/* ---- state halos ("deep halo"): exchange once per `depth` sweeps instead of once per sweep ---------------------------
 * The local graph of a rank additionally holds `depth` layers of its neighbours' variables (redundant copies, with all
 * their factors; beyond them a degree-1 stand-in per cut factor).  Between exchanges the handle runs plain cx_sweep calls;
 * an exchange overwrites every factor→variable message of the redundant variables with the values their owner holds.
 * After k <= depth sweeps every message of an OWNED variable equals the un-partitioned sweep's bit for bit: the error of
 * the frozen outer edge advances one layer per sweep and is wiped by the next exchange.  The redundant work is
 * 2*depth layers per rank; the per-sweep cost of the halo falls by the factor depth.
 *   cx_halo_configure_state : (variable, factor) of the messages exported to / imported from the neighbours, grouped by
 *                             peer like cx_halo_configure (cx_halo_peers, cx_halo_buffers, cx_halo_set_buffers apply).  Any dim:
 *                             a message travels in its storage form — 2 doubles (dim 1), d + d(d+1)/2 (dim 2..4: natural
 *                             parameters, packed symmetric), 64 + 64*64 (dim 64)
 *   cx_halo_state_pack / _unpack : gather into the send buffer / scatter from the recv buffer (caller-owned transport)
 *   cx_halo_state_exchange  : pack, grouped ncclSend/ncclRecv, unpack — all on the handle's stream (cx_comm_init first) */
int32_t cx_halo_configure_state(cx_handle *h, int64_t n_send, const int64_t *send_var, const int64_t *send_fac,
                                int64_t n_recv, const int64_t *recv_var, const int64_t *recv_fac);
/*   cx_halo_set_layers      : optional.  layer[i] = distance (1 .. depth; stand-ins depth + 1) of redundant variable_ids[i] from the
 *                             owned set.  cx_sweep then runs, in the j-th sweep after an exchange, only the slices that hold
 *                             variables of layer <= depth - j + 1 — the layers that can still be valid — instead of the whole local
 *                             graph (fused schedule).  Owned results are unchanged bit for bit. */
int32_t cx_halo_set_layers(cx_handle *h, int64_t n, const int64_t *variable_ids, const int32_t *layer, int32_t depth);
int32_t cx_halo_state_pack(cx_handle *h);
int32_t cx_halo_state_unpack(cx_handle *h);
int32_t cx_halo_state_exchange(cx_handle *h);
/*   cx_halo_exchange_sweep  : one batch = the exchange AND n_sweeps sweeps, the exchange overlapped with the first sweep: the slices
 *                             that hold owned variables only (known from cx_halo_set_layers) run on the handle's stream while a
 *                             second stream packs, sends / receives and unpacks; the redundant rows' part of that sweep follows the
 *                             unpack.  Bit-identical to cx_halo_state_exchange + cx_sweep(n_sweeps), and falls back to exactly that
 *                             when the handle cannot split a sweep (no layers, dim > 1, another schedule). */
int32_t cx_halo_exchange_sweep(cx_handle *h, int32_t n_sweeps);
/* The same exchange WITHOUT a collective library (dim 1 - 4): every rank pushes its boundary state straight into a receive area of
 * the neighbour — device memory the neighbour exported with hipIpcGetMemHandle — and raises an epoch flag there; the neighbour's
 * unpack kernel waits for the flag.  Two launches on the handle's stream per exchange (push; wait + unpack) instead of pack,
 * RCCL kernel, unpack.  Results are bit-identical to cx_halo_state_exchange.
 *   cx_halo_ipc_alloc     : after cx_halo_configure_state + cx_halo_peers.  Allocates this rank's block (flags + two receive areas)
 *                           and returns its 64-byte hipIpcMemHandle_t, its device address (for a neighbour in the SAME process,
 *                           which cannot open the handle) and the size of one receive area.  The caller carries the three to the
 *                           neighbours (torch.distributed.all_gather_object, MPI, a file).
 *   cx_halo_ipc_connect   : peer entry peer_index (order of cx_halo_peers) sends to the neighbour's block: handle64 XOR
 *                           same_process_base; remote_entry = the neighbour's peer entry that receives from this rank,
 *                           remote_recv_off = that entry's recv_offset (messages), remote_area_bytes = the neighbour's area size.
 *   cx_halo_ipc_push      : store the boundary state into the neighbours' receive areas of the next epoch, raise their flags
 *   cx_halo_ipc_unpack    : wait for this rank's flags of the epoch last pushed, scatter the receive area into the redundant rows
 *   cx_halo_ipc_exchange  : push, then unpack; asynchronous like cx_sweep.  Every neighbour has to call it the same number of
 *                           times.  A neighbour that does not arrive within the timeout (default 20 s) is NOT waited for for
 *                           ever: the unpack gives up, the grid drains and cx_halo_ipc_status reports it.
 *   cx_halo_ipc_status    : synchronises; *timed_out != 0 when an unpack gave up (results since are void), *exchanges = count */
int32_t cx_halo_ipc_alloc(cx_handle *h, void *handle64, void **local_base, int64_t *area_bytes);
int32_t cx_halo_ipc_connect(cx_handle *h, int32_t peer_index, const void *handle64, void *same_process_base, int32_t remote_entry,
                            int64_t remote_recv_off, int64_t remote_area_bytes);
int32_t cx_halo_ipc_push(cx_handle *h);
int32_t cx_halo_ipc_unpack(cx_handle *h);
int32_t cx_halo_ipc_exchange(cx_handle *h);
/*   cx_halo_ipc_exchange_sweep : one batch = push | the owned part of the first sweep | wait + unpack | the rest of that sweep |
 *                           sweeps 2 .. n, all on the handle's stream: the neighbours' pushes travel while this rank computes
 *                           its interior.  Bit-identical to cx_halo_ipc_exchange + cx_sweep(n), and exactly that when the sweep
 *                           cannot be split (no cx_halo_set_layers, dim > 1, another schedule). */
int32_t cx_halo_ipc_exchange_sweep(cx_handle *h, int32_t n_sweeps);
/*   cx_halo_ipc_batch     : one batch of n sweeps (2 <= n <= depth) with the push of the NEXT exchange inside its last sweep: that
 *                           sweep runs the slices that write the boundary state first, pushes, then runs the rest; the batch's own
 *                           exchange is unpacked after the owned part of its first sweep.  Between a push and the wait for it then
 *                           lie two partial sweeps of compute for the transfer to hide behind.  Bit-identical to
 *                           cx_halo_ipc_exchange + cx_sweep(n); afterwards the next exchange is pushed but not unpacked, which
 *                           cx_halo_ipc_exchange / _exchange_sweep / _batch pick up.  Falls back to cx_halo_ipc_exchange_sweep.
 *   cx_halo_ipc_set_fused : on != 0 — the caller asserts that every neighbour pushes from ANOTHER device: push and unpack of an
 *                           exchange may then share one launch.  Default off (two launches): a rank that is its own neighbour,
 *                           handles of one process and processes sharing a GPU must not wait inside a kernel for workgroups of the
 *                           same or a co-scheduled kernel. */
int32_t cx_halo_ipc_batch(cx_handle *h, int32_t n_sweeps);
int32_t cx_halo_ipc_set_fused(cx_handle *h, int32_t on);
int32_t cx_halo_ipc_status(cx_handle *h, int32_t *timed_out, int64_t *exchanges);
int32_t cx_halo_ipc_set_timeout(cx_handle *h, double seconds);

/* ---- partitioned chain scan (CX_SCHED_CHAIN_SCAN; SURVEY.md §8e: "contiguous time blocks + one composed map per block") ----
 * A rank holds a time block of a chain (its own variables, the cut transition factors, the remote end of each as a degree-1
 * stand-in named in cx_halo_configure).  The exact forward / backward messages of a block are a projective-linear function of
 * the ONE message that enters it at either end, so the ranks exchange maps, not sweeps:
 *   cx_chain_block_maps : the block's composed forward and backward maps over its links — 6 doubles each, (e f g A B C) of
 *                         [xi' w' 1] ~ [[e f g] [0 A B] [0 C 1]] [xi w 1] — and the side sums (all non-chain messages) of its
 *                         first and last variable, from the data currently on the device.  Before the call the caller sets the
 *                         factor→variable messages of the cut factors into the block's end variables to natural (0, 0), so that
 *                         the maps exclude them.
 *   [caller all-gathers the maps (16 doubles per rank), composes the prefixes and sets the stand-ins' variable→factor messages]
 *   cx_sweep(h, 1)      : the block's exact messages and marginals (cortex.jl_amd/partition.py: ChainScanExchange).
 * dim 2, 3, 4 (round 3): the same protocol with the maps of csrc/cx_mvchain.hip.  A map is ND = 2 d(d+1)/2 + d^2 + 2 d doubles —
 *   P (packed upper) | B (row-major) | C (packed upper) | h | c  of  f(eta, Lambda) = (c + B (Lambda + P)^-1 (eta + h), C - B (Lambda + P)^-1 B')
 *   — in forward6 / backward6 (ND doubles each); the side sums are eta[d] | Lambda (packed upper) in side_first2 / side_last2.  The
 *   stand-ins of a dim > 1 block are named with cx_halo_configure (recv lists only matter: they mark the stand-in variables).
 * dim 64 (round 4): the same layout (ND = 8,384, sides 2,144 doubles).  The block's composition tree (csrc/cx_mv64chain.hip) ends in
 *   ONE potential of its two end variables; the call runs the compose launches and returns it as the two directions' maps.  dim 64
 *   keeps one message buffer and no variable→factor messages, so the caller hands the boundary over AFTER the cut factor's rule: as
 *   the cut factor's factor→variable message into the block's end variable (cx_set_messages, CX_TO_VARIABLE).  A cx_sweep that
 *   follows with nothing but those two messages changed starts from the potentials that are on the device already (its walks only). */
int32_t cx_chain_block_maps(cx_handle *h, double *forward6, double *backward6, double *side_first2, double *side_last2,
                            int64_t *first_variable_id, int64_t *last_variable_id, int64_t *n_links);

/* ---- the chain-scan schedule for dim 64 (csrc/cx_mv64chain.hip) ----
 * One cx_sweep composes pairwise potentials of blocks of links bottom-up and walks them top-down (the plan: csrc/cx_chain64_plan.h),
 * so that ONE call is the reference's one update_marginals! on a chain (src/inference_engine.jl:575-608).  cx_chain_plan_stats
 * reports the plan the last cx_sweep used, for the work count of a measurement: out8 = {links per level-0 block, potentials per
 * group, levels, potentials, pairwise compositions per sweep (960 matrix instructions each), rule applications per sweep (384
 * each), kernel launches per sweep, device bytes of the plan}.  All zeros before the first sweep and for any other handle. */
int32_t cx_chain_plan_stats(const cx_handle *h, int64_t *out8);

/* CX_SCHED_TREE: the plan of the last sweep (zeros before the first one and for other schedules).
 * out8 = { depth, stages, items, k-ary entries, components, messages upwards, messages downwards, marginals }. */
int32_t cx_tree_plan_stats(const cx_handle *h, int64_t *out8);
/* CX_SCHED_TREE: when the sweep takes fewer launches that way, the plan runs over HEAVY PATHS — every variable's
 * heaviest child continues its path, through a two-edge factor or through a factor of more edges (which, given the messages of its
 * other variables, is a pairwise rule between the two: formed on the device before the depth's first scan); the paths of one light
 * depth (light edges above them) are ONE segmented scan per direction, whatever their length, the light edges stay items: O(log n)
 * rounds of launches instead of 2 x depth + 1 (a chain of T states with a latent layer below each: ~ 25 launches instead of ~ 2 T; a
 * tree of 1.1 M edges and 144,559 levels: 32).  The same messages, every marginal exact.
 * out4 = { light depths, paths of two or more variables, variables on no such path, launches per sweep }; zeros when the level
 * schedule is in use (then cx_tree_plan_stats's "stages" are its launches).  With heavy paths "stages" / "items" count the item stages. */
int32_t cx_tree_heavy_path_stats(const cx_handle *h, int64_t *out4);

/* ---- numerical guards as counters (non-finite values, variances <= 0 and matrices that are not positive definite are
 * reported through status codes and counters, never by an abort; the reference has nothing to mirror here — a rule that divides by
 * zero throws in the user's Julia code).  An undefined value is NaN and propagates by itself, a rule whose input is not positive
 * definite leaves its output undefined or unchanged; this call counts, on the device, the stored factor→variable messages INTO
 * NON-OBSERVED variables:  out4 = { defined, undefined (UndefValue: never computed, or a dependency was undefined), defined with a
 * negative precision (dim > 1: a diagonal entry of the precision matrix below -1e-12 times the largest diagonal entry of Q^-1 or
 * A' Q^-1 A of the pairwise rule that sends the message — a flat message, such as the one behind a forecast's end or a long run of
 * states without data, is the rounding of numbers of that size and is not counted; a message no pairwise rule sends is judged
 * strictly), defined with a non-finite entry (a point mass (y, +inf) of dim 1 is a value, not counted) }.  Synchronous. */
int32_t cx_message_health(cx_handle *h, int64_t *out4);

/* ---- log-evidence (ABI 5; no counterpart in the reference: its engine computes no numbers) ----
 * log p(data) of a CX_FAMILY_GAUSSIAN model, dim 1 - 4, from the STORED factor→variable messages and the caller's data (never the
 * marginals):  log Z = Σ_o c_o + Σ_a log z_a + Σ_i (1 - d_i) log z_i  over the opaque messages o (normalised densities when their
 * precision is positive definite), the Gaussian factors a (z_a = ∫ f_a Π m_{i→a}, observed variables fixed at their datum) and the
 * non-observed variables i (d_i = their factors that carry a rule; z_i = ∫ Π m_{a→i}).  Exact on forests at a fixed point — after one
 * chain-scan or tree sweep, one reference-order call that requested every variable, fused / flooding sweeps run to convergence — and
 * the Bethe estimate (minus the Bethe free energy) elsewhere.  A factor of zero noise (q = 0) is CX_ERR_UNSUPPORTED;
 * so are the other families, dim >= 5 and partitioned handles (halo lists, stand-in variables).  Works under every schedule the
 * handle accepts.
 * counts4 = {factor terms, variable terms (d_i != 1), terms with an undefined input, terms whose belief is not positive definite};
 * *value is NaN iff counts4[2] + counts4[3] > 0.  Synchronous; moves no message, marginal, readiness bit or counter. */
int32_t cx_log_evidence(cx_handle *h, double *value, int64_t *counts4);

/* ---- factor beliefs and EM statistics (ABI 6; no counterpart in the reference) ----
 * Both read what cx_log_evidence reads (the STORED factor→variable messages and the data; never the marginals), work after any
 * schedule, are exact on forests at a fixed point and give the Bethe factor beliefs elsewhere.  Covered: the
 * two-variable factors CX_FACTOR_GAUSS_ADDITIVE and CX_FACTOR_GAUSS_LINEAR of dim 1, CX_FACTOR_GAUSS_LINEAR of dim 2 - 4.  Refused
 * exactly as cx_log_evidence refuses (other families, dim >= 5, partitioned handles, zero-noise factors, a captured stream).
 * Out of scope: dims 5 - 64, factors of more than two variables (CX_FACTOR_GAUSS_LINEAR_N), variational families.
 * Synchronous; they move no message, marginal, readiness bit or counter.
 *
 * cx_factor_beliefs: the joint Gaussian posterior of each named factor's two variables.  out: n rows of 2d + (2d)^2 doubles, the
 * 2d means then the 2d x 2d covariance, row-major, in the order (out, in): CX_ROLE_OUT then CX_ROLE_IN; CX_FACTOR_GAUSS_ADDITIVE
 * (no roles) takes the edge of the lower variable id as `out`.  An observed variable's entries are its datum with zero rows and
 * columns in the covariance.  A factor with an undefined input, or whose belief is not positive definite, reads as NaN.
 * An unknown id is CX_ERR_NOT_FOUND; any other factor kind is CX_ERR_UNSUPPORTED (naming it).  At dim 1 this is the stored-message
 * counterpart of a scheduled CX_ITEM_JOINT_MARGINAL (cx_get_joint_marginals).
 */
int32_t cx_factor_beliefs(cx_handle *h, int64_t n, const int64_t *factor_ids, double *out);

/* cx_factor_statistics: the expected sufficient statistics of EM (Shumway–Stoffer), summed per group of factors that share A, in
 * RESIDUAL coordinates r = x_out - A x_in - b under the factor's current parameters (dim 1: (a, b) of CX_FACTOR_GAUSS_LINEAR, (1, 0)
 * of CX_FACTOR_GAUSS_ADDITIVE; dim 2 - 4: the parameter set's A and the factor's own b — cx_set_factor_offsets, 0 unless set; factors of
 * one group may differ in b, as they may in q at dim 1).  out: n_groups rows of 1 + 2d + 3d^2 doubles,
 *     n_g | Σ E[r] (d) | Σ E[x_in] (d) | Σ E[r r'] (d x d) | Σ E[r x_in'] (d x d) | Σ E[x_in x_in'] (d x d)     (row-major)
 * from which the M-step is  ΔA = S_rx S_xx^-1,  A' = A + ΔA,  Q' = (S_rr - ΔA S_rx') / n_g  (a Q-only update: Q' = S_rr / n_g).
 * Sums are compensated (f64) and taken in a fixed order: two calls on one state are bit-identical.
 * Grouping:
 *   factor_ids == NULL (and groups == NULL; n is ignored), dim 2 - 4: the group of a factor is its parameter set; every
 *     CX_FACTOR_GAUSS_LINEAR factor counts; n_groups must exceed the largest set in use (rows of unused sets: zeros, n_g = 0).
 *     A set also read by a CX_FACTOR_GAUSS_LINEAR_N factor (its own or an edge set of cx_set_factor_edge_sets) is
 *     CX_ERR_UNSUPPORTED: its statistics would be incomplete.  At dim 1 a NULL factor_ids is CX_ERR_INVALID_ARGUMENT.
 *   factor_ids, groups (length n): factor factor_ids[i] goes to row groups[i] (-1: skipped).  A group's factors must share their A
 *     (dim 2 - 4: one parameter set; dim 1: the same kind, a and b; q may differ), else CX_ERR_INVALID_ARGUMENT naming two of them;
 *     a factor listed twice is CX_ERR_INVALID_ARGUMENT; an unknown id CX_ERR_NOT_FOUND; a factor of another kind CX_ERR_UNSUPPORTED.
 * The work list of the last grouping is cached: a call with the same arrays costs an O(n) comparison on the host; a new grouping is
 * checked and its lists built and uploaded (O(n + n_groups) on the host).
 * counts4 = {factors counted, non-empty groups, factors with an undefined input, factors whose belief is not positive definite};
 * a group's row is NaN (n_g excepted) when one of its factors is counted in either of the last two. */
int32_t cx_factor_statistics(cx_handle *h, int64_t n, const int64_t *factor_ids, const int64_t *groups, int64_t n_groups, double *out,
                             int64_t *counts4);

/* ---- joint posterior samples (ABI 7; no counterpart in the reference) ----
 * cx_sample_posterior: n_samples joint draws of the non-observed variables of a Gaussian forest — the simulation smoother (forward
 * filtering, backward sampling) on any forest, dim 1 - 4.  Each component of the forest of non-observed variables is
 * rooted where the tree schedule's heavy-path plan roots it (an end of a longest path) and drawn from
 *     q(x) = b_r(x_r) Π_a b_a(x_{C_a} | x_{p_a}),
 * b_r the root's belief (the sum of its stored factor→variable messages), b_a the factor belief of cx_factor_beliefs (§4e / §4f), p_a
 * the factor's variable nearest the root and C_a its other non-observed variables (drawn jointly; up to 6 for a k-ary factor).
 * It reads what cx_log_evidence reads (the STORED messages and the data, never the marginals).  At a fixed point on a forest q is
 * exactly p(x | data), whatever the root; when the messages are not at a fixed point q is still a proper distribution, but it depends
 * on the root.  Covered: CX_FACTOR_GAUSS_ADDITIVE, CX_FACTOR_GAUSS_LINEAR and CX_FACTOR_GAUSS_LINEAR_N (3 - 7 edges) at dim 1,
 * CX_FACTOR_GAUSS_LINEAR and CX_FACTOR_GAUSS_LINEAR_N at dim 2 - 4, opaque messages as part of each variable's sum.
 * out: a host array [n_samples][n][dim] (row-major) for variable_ids (NULL: every variable in ascending id; n is ignored).  An
 * observed variable's rows hold its datum.  Every row of a component with an undefined input, or whose root belief or a conditional
 * precision J_CC is not positive definite, is NaN; other components are unaffected.  A non-observed variable on no factor is NaN.
 * noise == NULL: the standard normals come from Philox4x32-10 on the device, counter (j, v, s mod 2^32, s / 2^32), key (seed mod 2^32,
 * seed / 2^32), for components 2j and 2j + 1 of the variable of index v (ascending id order) in sample s; the four words give two
 * uniforms u = (w53 + 0.5) 2^-53 from (word 1 << 32 | word 0) >> 11 and (word 3 << 32 | word 2) >> 11, and Box–Muller:
 * ε_2j = sqrt(-2 ln u1) cos(2π u2), ε_2j+1 = sqrt(-2 ln u1) sin(2π u2).  A draw does not depend on n_samples, variable_ids or the launch.
 * noise != NULL: the caller's ε, a host array [n_samples][n_variables][dim] in ascending variable-id order (n_variables of
 * cx_graph_stats; the rows of observed variables are ignored); the call is then a fixed affine map of ε.
 * counts4 = {free variables sampled, components, components with an undefined input, components not positive definite}.
 * Refused as cx_log_evidence refuses, with the same codes (other families, dim >= 5, partitioned handles, zero-noise factors, a
 * captured stream); a cycle among the non-observed variables is CX_ERR_UNSUPPORTED; n_samples < 1, a NULL out or counts4, or n < 0
 * with ids is CX_ERR_INVALID_ARGUMENT; an unknown id CX_ERR_NOT_FOUND.  The plan is cached and rebuilt when the graph or the observed
 * flags change.  Synchronous; moves no message, marginal, readiness bit or counter. */
int32_t cx_sample_posterior(cx_handle *h, int64_t n_samples, uint64_t seed, const double *noise, int64_t n, const int64_t *variable_ids,
                            double *out, int64_t *counts4);

/* ---- predictive scores of the data (ABI 8; no counterpart in the reference) ----
 * cx_predictive: for every observation that a Gaussian rule factor generates, the predictive distribution of that datum given other
 * data, its log score and its squared standardised residual — the leave-one-out cross-validation terms, or the innovations of the
 * prediction-error decomposition.  Dim 1 - 4, CX_FAMILY_GAUSSIAN.  It reads what cx_log_evidence reads (the STORED
 * factor→variable messages and the caller's data, never the marginals) and works after every schedule the handle accepts.
 * A ROW is a rule factor a,  y = Σ_i A_i x_i + b + N(0, Q),  whose CX_ROLE_OUT end is observed (the datum y) and whose other ends are
 * all non-observed: CX_FACTOR_GAUSS_LINEAR, CX_FACTOR_GAUSS_LINEAR_N (3 - 7 edges), and CX_FACTOR_GAUSS_ADDITIVE at dim 1 with either
 * end observed (it is symmetric).  For every input i the cavity  m_{i\a} = M_i - m_{a→i} - (what the mode leaves out),  M_i the sum of
 * ALL stored messages into i (the opaque ones included), has mean μ_i^c and covariance Σ_i^c, and
 *     ŷ = Σ_i A_i μ_i^c + b,   S = Σ_i A_i Σ_i^c A_i' + Q,   log_density = log N(y; ŷ, S),   maha = (y - ŷ)' S^-1 (y - ŷ).
 * Exact on a forest at a fixed point (the cavities of distinct inputs are independent once a is removed), the cavity (Bethe)
 * approximation elsewhere.
 *   CX_PREDICT_LOO     nothing is left out but the factor's own message: p(y_a | all other data).  Σ log_density is the leave-one-out
 *                      cross-validation score.
 *   CX_PREDICT_CAUSAL  also left out of input i's cavity: every message into i from a rule factor on which i is a CX_ROLE_IN end — what
 *                      flows back from what i generates (its other observations, its successors).  CX_FACTOR_GAUSS_ADDITIVE has no
 *                      roles: as in cx_factor_beliefs the lower variable id is `out`, the higher `in`.  On a chain with at most one
 *                      observation per state this is the one-step-ahead prediction p(y_t | y_<t): the rows are the Kalman innovations
 *                      (ŷ_t, S_t) and Σ log_density equals cx_log_evidence.  On a chain of CX_FACTOR_GAUSS_ADDITIVE transitions (ids
 *                      ascending in time) it is the reverse-time filter p(y_t | y_>t), with the same sum.  On a branching graph a row
 *                      conditions on the data of its inputs' ancestors only, and the sum is NOT the evidence.
 * Rows: factor_ids == NULL: every row in ascending factor id (n is ignored; cx_predictive_rows names them); otherwise the n named
 * factors in the caller's order — an unknown id is CX_ERR_NOT_FOUND, a factor that is not a row CX_ERR_UNSUPPORTED (naming it).
 * out: NULL, or a host array of counts4[0] rows of d + d^2 + 2 doubles:  ŷ[d] | S[d][d] (row-major) | log_density | maha.  A row with
 * an undefined (NaN) input is NaN; a row whose cavity or S is not positive definite — an improper predictive, such as the first
 * observation of a chain without a prior, which the Kalman decomposition also leaves out — is NaN and counted apart (a cavity from
 * which every message into the variable is taken out is improper by structure, whatever the subtraction rounds to; so is one whose
 * cavity has a Cholesky pivot below 64 ulp of the belief's own diagonal entry: what a flat message left behind, such as the one
 * behind a forecast's end, is the rounding of the subtraction, of either sign).
 * counts4 = {rows, rows scored, rows with an undefined input, rows improper} (never NULL; a call with out == NULL sizes the array).
 * *total (may be NULL): the compensated f64 sum of log_density over the SCORED rows only, in a fixed order: two calls on one state are
 * bit-identical.  With out == NULL only the total and the counters come back (a learning loop's objective).
 * The rows of the last (mode, factor_ids) are cached: the same call again costs an O(n) comparison on the host; they are rebuilt when
 * the graph or the observed flags change; rule parameters are re-read when they change.
 * Refused as cx_log_evidence refuses, with the same codes (other families, dim >= 5, partitioned handles, zero-noise factors, a
 * captured stream); an unknown mode, a NULL counts4 or n < 0 with ids is CX_ERR_INVALID_ARGUMENT.  Out of scope: a datum on the
 * CX_ROLE_IN end of a non-additive factor.  Synchronous; moves no message, marginal, readiness bit or counter.
 *
 * cx_predictive_rows: the factor ids of the rows a NULL factor_ids scores, ascending: *n_rows of them, the first min(cap, *n_rows)
 * written to factor_ids (cap == 0: factor_ids may be NULL).  Host work only; refused as cx_predictive. */
#define CX_PREDICT_LOO 0
#define CX_PREDICT_CAUSAL 1
int32_t cx_predictive(cx_handle *h, int32_t mode, int64_t n, const int64_t *factor_ids, double *out, double *total, int64_t *counts4);
int32_t cx_predictive_rows(cx_handle *h, int64_t cap, int64_t *factor_ids, int64_t *n_rows);

/* ---- exact moments of linear functionals (ABI 9; no counterpart in the reference) ----
 * cx_linear_moments: the mean and the covariance of K linear functionals  φ_k(x) = Σ_i w_{k,i}' x_i  of the joint posterior of a Gaussian
 * forest, dim 1 - 4: the variance of x_i - x_j for two states far apart, of a window average of a smoothed chain, the
 * covariance of two regional totals on a tree, the lag-k autocovariance of a smoother — what no marginal and no factor belief holds.
 * The setting is cx_sample_posterior's: the forest of non-observed variables, rooted the same way, the same q(x), read from the STORED
 * factor→variable messages and the data (never the marginals), after any schedule.  A draw is x = c + z⁰ + F ε (§4g), so
 *     mean[k] = φ_k of the draw with ε = 0,      cov = W F F' W'  (W: the weights on the non-observed variables),
 * and F' is the sampler's scan run leaf-to-root, on the device, for all K at once: exact at a fixed point on a forest (q = p there), the
 * moments of the same q the sampler draws from elsewhere.  Nothing of size n is copied to the host.
 * The functionals come sparse, in CSR form: functional k has the entries offsets[k] .. offsets[k + 1] - 1 (offsets[0] = 0, never
 * decreasing) of variable_ids and of weights ([nnz][dim], row-major).  A variable named more than once within a functional counts with
 * the sum of its weights.  An observed variable adds w' datum to the mean and nothing to cov.
 * mean: a host array [K].  cov: NULL (the means only; the leaf-to-root scan is skipped) or a host array [K][K], symmetric by
 * construction (one triangle is computed and mirrored).  A functional that touches a component with an undefined input, or whose root
 * belief or a conditional precision is not positive definite (cx_sample_posterior's status), has a NaN mean and a NaN row and column
 * of cov; the others are unaffected.  counts4 = {components, failed components, functionals made NaN, non-observed variables}.
 * A functional's numbers do not depend on which others share the call, nor on how the call is cut into chunks of functionals; every
 * sum is compensated and in a fixed order: two calls on one state are bit-identical.  The noise coordinates of all K functionals are
 * kept on the device, K x (non-observed variables) x dim doubles: past 2^30, or past 2^28 partial sums (K x K per 2048 variables),
 * the call is refused with CX_ERR_OUT_OF_MEMORY (ask for fewer functionals per call; cov == NULL has no such bound).
 * Refused as cx_sample_posterior refuses, with the same codes (other families, dim >= 5, partitioned handles, zero-noise factors, a
 * captured stream; a cycle among the non-observed variables is CX_ERR_UNSUPPORTED); n_functionals < 0 or above 32768, a NULL offsets,
 * mean or counts4, NULL variable_ids or weights with entries, or offsets that do not start at 0 or decrease are
 * CX_ERR_INVALID_ARGUMENT; an unknown id CX_ERR_NOT_FOUND.  Shares the sampler's cached plan.  Synchronous; moves no message, marginal,
 * readiness bit or counter. */
int32_t cx_linear_moments(cx_handle *h, int64_t n_functionals, const int64_t *offsets, const int64_t *variable_ids, const double *weights,
                          double *mean, double *cov, int64_t *counts4);

/* ---- causal marginals of the states (added after ABI 9: a new function breaks no caller, CX_ABI_VERSION stays; no counterpart in the
 * reference) ----
 * cx_causal_marginals: beside the smoothed marginals of cx_get_marginals, p(x_i | all data), the estimates a real-time user reports:
 * the one-step prediction p(x_t | y_<t), the filtered estimate p(x_t | y_<=t) and the fixed-lag smoother p(x_t | y_<=t+L), dim 1 - 4
 * (DESIGN.md §4j), from the STORED factor→variable messages, the rule parameters and the data (never the marginals), after any schedule.
 * Every stored message into a non-observed variable i is of one class — cx_predictive's conventions, so that the two calls agree:
 *   U_i  upstream: the message of an opaque (caller-set) factor, or of a rule factor on which i is not a CX_ROLE_IN end
 *   O_i  i's own observations: of a rule factor on which i is a CX_ROLE_IN end and whose CX_ROLE_OUT end is observed; of a
 *        CX_FACTOR_GAUSS_ADDITIVE factor (dim 1) whose other end is observed, whichever id is lower
 *   T_i  transitions onward: of a rule factor on which i is a CX_ROLE_IN end and whose CX_ROLE_OUT end is not observed
 *        (CX_FACTOR_GAUSS_ADDITIVE has no roles: the lower variable id is `out`, as in cx_factor_beliefs and cx_predictive)
 * and the result is a sum of messages, in natural parameters:
 *   CX_CAUSAL_PREDICTED (lag 0)   Σ U_i
 *   CX_CAUSAL_FILTERED, lag 0     Σ U_i + Σ O_i
 *   CX_CAUSAL_FILTERED, lag L     Σ U_i + Σ O_i + Σ_{a in T_i} β_a^(L),  with β_a^(0) flat and, for the transition a with `out` end j,
 *                                 β_a^(s) = the factor's sum-product rule towards i applied to Σ O_j + Σ_{a' in T_j} β_a'^(s-1):
 *                                 the backward message that has seen only the data within L transitions downstream.
 * On a chain with a prior or data at its start these are the Kalman predicted, filtered and fixed-lag-smoothed states (a chain of
 * CX_FACTOR_GAUSS_ADDITIVE transitions with ids ascending in time: their reverse-time counterparts, as cx_predictive documents); on any
 * forest at a fixed point p(x_i | every datum except those of i's descendants [+ i's own] [+ of descendants within L transitions]); on a
 * loopy graph the same formula on the Bethe messages; with L at least the depth below i, the smoothed marginal.  The sums are sums of
 * the messages kept, never the belief minus what is left out: nothing cancels.
 * Rows: variable_ids == NULL: every variable in ascending id (n is ignored; cx_graph_stats gives n_variables); otherwise the n named
 * variables in the caller's order.  out: a host array [rows][dim + dim²], mean then covariance (row-major), the moment form of
 * cx_get_marginals.  An observed variable's row is its datum and a zero covariance.  A row that read an undefined (NaN) message is NaN; a
 * row whose precision is not positive definite — nothing kept at all, such as the predicted first state of a chain without a prior — is
 * improper and NaN.  counts4 = {rows, rows returned finite, rows with an undefined input, rows improper}.  A variable's numbers do not
 * depend on which others share the call; two calls on one state are bit-identical.
 * Cost: one pass over the messages and one thread per row; a lag L adds L passes over EVERY transition of the graph, whatever rows are
 * asked for.  The classes and the transition list are built on the first call and again after the graph or the observed flags changed.
 * Refused as cx_log_evidence refuses, with the same codes (other families, dim >= 5, partitioned handles, zero-noise factors, a captured
 * stream, no graph); an unknown mode, lag < 0, lag > 0 with CX_CAUSAL_PREDICTED, a NULL out or counts4, or n < 0 with ids are
 * CX_ERR_INVALID_ARGUMENT; an unknown id CX_ERR_NOT_FOUND; lag > 0 on a graph that holds a transition through a
 * CX_FACTOR_GAUSS_LINEAR_N factor (a free CX_ROLE_OUT end and a free CX_ROLE_IN end: the recursion has no single predecessor there) is
 * CX_ERR_UNSUPPORTED and names the factor — with lag 0 such factors are simply classified as above.  Synchronous; moves no message,
 * marginal, readiness bit or counter. */
#define CX_CAUSAL_PREDICTED 0
#define CX_CAUSAL_FILTERED 1
int32_t cx_causal_marginals(cx_handle *h, int32_t mode, int32_t lag, int64_t n, const int64_t *variable_ids, double *out, int64_t *counts4);

/* ---- per-factor offsets, dim 2 - 4 (added after ABI 9: a new function breaks no caller, CX_ABI_VERSION stays; the reference has no
 * d-dimensional rule at all) ----
 * cx_set_factor_offsets: the two-variable CX_FACTOR_GAUSS_LINEAR factors named become x_out = A x_in + b + N(0, Q) with b = offsets[i]
 * (offsets: [n][dim], row-major) — a control input B u_t, a drift, an observation mean, a regression effect: whatever enters a factor as
 * a constant.  (A, Q) stay the parameter set's.  Offsets of factors not named keep their value; the initial value is 0; a later call
 * replaces the named factors' offsets; n == 0 changes no offset and still marks the handle as having offsets.
 * What it does: the factor's potential gains the linear terms g_out = Q^-1 b, g_in = -A' Q^-1 b; every message from the
 * sending end s to the receiving end p keeps its precision and has eta_p = g_p + B (Lambda_s + P)^-1 (eta_s + g_s) (an observed sender:
 * eta_p = g_p + B y, the message N(A y + b, Q)).  Covered: CX_SCHED_FUSED (degree > 8 and damping included), CX_SCHED_CHAIN_SCAN
 * (marginals and messages on demand included), CX_SCHED_TREE (level plans, heavy paths, the captured sweep), cx_update_batch message
 * items, cx_residual / cx_sweep_until, and of the derived calls cx_log_evidence, cx_factor_beliefs, cx_factor_statistics (r uses the
 * factor's own b) and cx_predictive (y^ = A mu + b).  cx_sample_posterior, cx_linear_moments and cx_causal_marginals return
 * CX_ERR_UNSUPPORTED, naming this function, while any offset is non-zero, and work as before once all are 0 again.
 * cx_set_factor_matrices afterwards keeps b and recomputes the linear terms.  The offsets are rule parameters: part of the checkpoint
 * fingerprint once the function has been called (a blob taken under other offsets, or none, is refused; handles that never called it
 * exchange blobs as before).
 * A handle on which the function was never called launches the kernels it always launched; a handle whose offsets are all 0 computes the
 * same numbers (==) through the offset instances of the kernels.
 * Refused: dim 1 CX_ERR_STATE (dim 1 factors carry b in their parameters); dim 5 - 64 (cx_set_factor_offsets_mfma is theirs), other families, CX_SCHED_REFERENCE handles (wired
 * or not: the reference order has nothing to pin a d-dimensional offset against), a partitioned handle (halo lists, state halos, a
 * chain's time block — and configuring a halo or asking for block maps on a handle that has offsets) CX_ERR_UNSUPPORTED; a factor of
 * another kind (CX_FACTOR_GAUSS_LINEAR_N included) CX_ERR_UNSUPPORTED, naming it; an unknown id CX_ERR_NOT_FOUND; a non-finite entry,
 * n < 0 or NULL arrays with n > 0 CX_ERR_INVALID_ARGUMENT; no graph or a captured stream CX_ERR_STATE.  A refused call changes nothing.
 * Synchronous. */
int32_t cx_set_factor_offsets(cx_handle *h, int64_t n, const int64_t *factor_ids, const double *offsets);

/* ---- per-factor offsets, dim 5 - 64 (added after ABI 9: a new function breaks no caller, CX_ABI_VERSION stays) ----
 * cx_set_factor_offsets_mfma: cx_set_factor_offsets for a handle of dim 5 - 64 — a state-space model with a control input B u_t, a drift
 * or an observation mean y = H x + c + v at d = 16.  offsets: [n][the user's dim], row-major (an embedded dim, 5 - 15, 17 - 31, 33 - 63:
 * the caller's rows; nothing of b reaches the identity block of the padding).  The contract is cx_set_factor_offsets' own: offsets of
 * factors not named, the initial value 0, n == 0, finite values only, unknown id, factor of another kind, captured stream, no graph, the
 * checkpoint fingerprint, and what cx_set_factor_matrices afterwards does.
 * What it does: the linear terms g_out = Q^-1 b, g_in = -A' Q^-1 b are kept per message slot as one contiguous vector
 * each; the wave-per-message rule takes g of the sender's slot into its input eta and g of the destination slot into its output (its
 * offset instances; an observed sender: eta_p = g_p + B y), the chain plans name the same vectors as the h and c of a link's potential.
 * Covered: CX_SCHED_FUSED (senders of degree 5 - 8 and damping included), CX_SCHED_CHAIN_SCAN, CX_SCHED_TREE (level plans, heavy paths,
 * the captured sweep), cx_update_batch message items, cx_get_marginals / cx_get_messages / cx_get_products / cx_residual (they read
 * messages), and of the derived calls cx_log_evidence_mfma, cx_log_evidence_components_mfma, cx_factor_beliefs_mfma and
 * cx_factor_statistics_mfma (r = x_out - A x_in - b with the factor's own b).  cx_predictive_mfma, cx_predictive_rows_mfma,
 * cx_causal_marginals_mfma, cx_sample_posterior_mfma and cx_linear_moments_mfma return CX_ERR_UNSUPPORTED, naming this function, while any
 * offset is non-zero, and work as before once all are 0 again: no call computes as if b were 0.
 * A handle on which the function was never called launches the kernels it always launched; a handle whose offsets are all 0 computes the
 * same numbers (==) through the offset instances.
 * Refused: dim 1 - 4 CX_ERR_UNSUPPORTED (naming cx_set_factor_offsets); other families, CX_SCHED_REFERENCE handles, a partitioned handle
 * (and configuring a halo or asking for block maps afterwards) CX_ERR_UNSUPPORTED; the argument errors of cx_set_factor_offsets.  A
 * refused call changes nothing.  Synchronous. */
int32_t cx_set_factor_offsets_mfma(cx_handle *h, int64_t n, const int64_t *factor_ids, const double *offsets);

/* ---- connected components and the log-evidence of each (added after ABI 9: a new function breaks no caller, CX_ABI_VERSION stays; no
 * counterpart in the reference) ----
 * One handle may hold many independent models (a panel of series, K replicas of one series under K candidate parameter sets): the
 * connected components of the bipartite graph exactly as cx_graph_create received it.  Two variables are in one component when a path
 * of connections joins them; observed variables and opaque factors count like any other node, so the components depend on the graph
 * alone, not on which variables are observed — an observed variable shared by two otherwise separate models joins them into ONE
 * component.  Components are numbered 0 .. C-1 by their least variable id, ascending; a factor belongs to the component of its
 * variables.
 *
 * cx_graph_components: component[i] = the component of variable_ids[i]; variable_ids == NULL: every variable in ascending id (n is
 * ignored; cx_graph_stats gives n_variables).  component may be NULL when only *n_components is wanted.  Host work only (a union-find
 * over the connections per call, O(connections); a lookup once cx_log_evidence_components has built its plan on the handle); every dim
 * (1 - 64) and schedule once a graph exists.  No graph: CX_ERR_STATE; an unknown id:
 * CX_ERR_NOT_FOUND, naming it; a NULL n_components or n < 0 with ids: CX_ERR_INVALID_ARGUMENT; the variational families keep their
 * graph in another form: CX_ERR_UNSUPPORTED.
 *
 * cx_log_evidence_components: values[k] = the sum of exactly the terms of cx_log_evidence that belong to component k — the variable
 * terms, the centred opaque terms that travel with them, the factor terms of two-variable and k-ary factors — from the same STORED
 * messages.  It writes the first min(cap, C) entries of values and of comp_counts4 and *n_components = C;
 * comp_counts4 may be NULL, otherwise it is [cap][4] with the meaning of cx_log_evidence's counts4 restricted to the component;
 * cap == 0 with NULL arrays is the sizing call.  values[k] is NaN iff component k has a term with an undefined input or a belief that
 * is not positive definite: the other components keep their values (cx_log_evidence's one total would be NaN).  counts4 is the whole
 * graph's, equal to what cx_log_evidence returns.  The terms are summed per component on the device, compensated and in an order that
 * the graph alone fixes (no atomics): two calls on one state are bit-identical, a value does not depend on cap, and the sum of the
 * values agrees with cx_log_evidence to the rounding of two orders of summation, not bit for bit.
 * The labels, the terms sorted by component and the segment offsets are built on the first call (O(connections) on the host) and kept
 * with cx_log_evidence's work lists.  Refused as cx_log_evidence refuses, with the same codes (other families, dim >= 5, partitioned
 * handles, zero-noise factors, a factor without a rule, a captured stream, no graph); a NULL n_components or counts4, cap < 0, or
 * cap > 0 with a NULL values are CX_ERR_INVALID_ARGUMENT.  Synchronous; moves no message, marginal, readiness bit or counter. */
int32_t cx_graph_components(cx_handle *h, int64_t n, const int64_t *variable_ids, int64_t *component, int64_t *n_components);
int32_t cx_log_evidence_components(cx_handle *h, int64_t cap, double *values, int64_t *comp_counts4, int64_t *n_components, int64_t *counts4);

/* ---- log-evidence at the matrix-core dims (added after ABI 9: a new function breaks no caller, CX_ABI_VERSION stays; no counterpart
 * in the reference) ----
 * log p(data) of a CX_FAMILY_GAUSSIAN model at the matrix-core dims (cx_create dim 5 .. 64), from the STORED factor→variable
 * messages and the caller's data: the formula, the meaning of counts4 and the NaN rule of cx_log_evidence,
 *     log Z = sum_o c_o + sum_a log z_a + sum_i (1 - d_i) log z_i,
 * counts4 = {factor terms, variable terms (d_i != 1), terms with an undefined input, terms whose belief is not positive definite},
 * *value NaN iff counts4[2] + counts4[3] > 0.  Exact on forests at a fixed point, the Bethe estimate on loops; after every schedule
 * these dims accept (fused, chain scan, tree, reference order).  Only two-variable CX_FACTOR_GAUSS_LINEAR factors and opaque messages
 * exist at these dims.  Every term is one or two Cholesky factorisations of a "rule table + sum of message records" matrix by one
 * wave on the f64 matrix cores: a leave-one-out message is the sum of the variable's OTHER stored messages (never a
 * difference), a factor with two free ends eliminates its OUT end first (positive definite whenever the input is defined, a flat leaf
 * included) and keeps the resulting message in registers, an opaque message that is not positive definite (a flat forecast end)
 * contributes 0 and counts as no failure.  counts4[2] counts terms with a NaN input (a message record or a datum), counts4[3] terms
 * whose inputs are defined and one of whose factorisations meets a non-positive pivot — the first one of a factor with two free ends
 * included.  A dim of 5 .. 15, 17 .. 31 or 33 .. 63 runs embedded in the next tile size (cx_create): every log-determinant and
 * quadratic form is restricted to the real block and d is the caller's, so the value is the real model's at any internal tile size.
 * The terms are evaluated around the origin, NOT centred on the belief means as cx_log_evidence's are: about 1e-9 relative is lost once
 * the data lie some 3e3 sqrt(d) standard deviations from the origin (an estimate from the size of the terms that cancel, not a
 * measurement).  The terms are summed in an order the graph alone fixes (no atomics): two calls on one state are bit-identical.
 * The term lists are built on the first call (O(connections) on the host) and kept until other variables are observed; log det 2 pi Q
 * per parameter set follows cx_set_factor_matrices.  MI355X (profiles/evidence_mfma.md, session of 2026-10-19): T = 1e5 chains after
 * one chain-scan sweep, median of 30 calls: 4.68 ms at d = 64 (config C5), 1.51 ms at d = 32, 0.73 ms at d = 16 — 1.16, 1.36 and 1.65
 * times one fused sweep of the same model (4.05, 1.11, 0.44 ms): the call factors 4 T matrices where that sweep factors 2 T.
 * cx_log_evidence and cx_log_evidence_components keep returning CX_ERR_UNSUPPORTED at these dims exactly as before; routing them here
 * is a later, separate decision (the per-component call at these dims is cx_log_evidence_components_mfma, below).
 * Refused: NULL value or counts4 CX_ERR_INVALID_ARGUMENT; no graph or a captured stream CX_ERR_STATE; a handle created with dim 1 - 4
 * (use cx_log_evidence), other families, a factor of another kind, partitioned handles (halo lists, state halos, a chain's time
 * block) CX_ERR_UNSUPPORTED; wired handles (cx_graph_wire) cannot exist at these dims.  Synchronous; moves no message, marginal,
 * readiness bit or counter. */
int32_t cx_log_evidence_mfma(cx_handle *h, double *value, int64_t *counts4);

/* ---- log-evidence per connected component at the matrix-core dims (added after ABI 9; no counterpart in the reference) ----
 * cx_log_evidence_components_mfma: cx_log_evidence_components for a handle created with dim 5 .. 64 — the same arguments, outputs,
 * counts and NaN rule (see "cx_log_evidence_components" above and DESIGN.md §4t).  values[k] = the sum of exactly the terms of
 * cx_log_evidence_mfma that belong to component k (an opaque term belongs to its variable's component, a factor term to its
 * factor's); NaN iff one of those terms has an undefined input or is not positive definite, the other components keep their values
 * (cx_log_evidence_mfma's one total would be NaN).  comp_counts4 (NULL, or [cap][4]) = {factor terms, variable terms, undefined, not
 * positive definite} of every component; counts4 is cx_log_evidence_mfma's for the whole graph, the column sums of the components'.
 * Components are numbered as cx_graph_components numbers them.  It writes the first min(cap, C) entries and *n_components = C; cap == 0
 * with NULL arrays is the sizing call; values and counts4 do not depend on cap.
 * The device work is cx_log_evidence_mfma's term kernel (one wave per term, the same launch), then the segmented sum of
 * cx_log_evidence_components over the term array: compensated, in an order that a component's own terms fix, no atomics — two calls on
 * one state are bit-identical, a component's value does not depend on which others share the graph, and the sum of the values agrees
 * with cx_log_evidence_mfma to the rounding of two orders of summation, not bit for bit.  The labels and the sorted positions are
 * built on the first call (O(connections) on the host) and kept with cx_log_evidence_mfma's term lists, until other variables are
 * observed.  MI355X (profiles/evidence_components_mfma.md, session of 2026-10-21), medians of 30 calls interleaved with
 * cx_log_evidence_mfma on the same handle: 1.001, 1.007 and 1.001 times that call on a T = 1e5 chain at d = 16, 32 and 64 (0.69, 1.49,
 * 4.65 ms), 0.995 times on 1000 chains of T = 100 at d = 16.
 * Refused as cx_log_evidence_mfma refuses, with the same codes (a handle created with dim 1 - 4: use cx_log_evidence_components; other
 * families, a factor of another kind, partitioned handles CX_ERR_UNSUPPORTED; no graph or a captured stream CX_ERR_STATE); a NULL
 * n_components or counts4, cap < 0, or cap > 0 with a NULL values are CX_ERR_INVALID_ARGUMENT.  A refused call writes nothing.
 * Synchronous; moves no message, marginal, readiness bit or counter. */
int32_t cx_log_evidence_components_mfma(cx_handle *h, int64_t cap, double *values, int64_t *comp_counts4, int64_t *n_components, int64_t *counts4);

/* ---- factor beliefs and EM statistics at the matrix-core dims (added after ABI 9; no counterpart in the reference) ----
 * cx_factor_beliefs_mfma / cx_factor_statistics_mfma: cx_factor_beliefs and cx_factor_statistics for a handle created with dim 5 .. 64 —
 * the same contract, row layouts, roles (out, in), grouping rules, counts and NaN rule (see there and DESIGN.md §4f), with d the
 * CALLER's dim: a belief row is 2d + (2d)^2 doubles, a statistics row 1 + 2d + 3d^2.  A dim embedded in the next tile size (5 .. 15 in
 * 16, 17 .. 31 in 32, 33 .. 63 in 64, or one forced by CX_MFMA_DIM) returns the real block only, with the real model's values at any
 * internal tile size.  Covered: the two-variable CX_FACTOR_GAUSS_LINEAR factor with either, both or none of its ends observed; opaque
 * messages are part of each variable's sum.  r = x_out - A x_in - b with the factor's own b (cx_set_factor_offsets_mfma; 0 unless set).  They read what
 * cx_log_evidence_mfma reads (the STORED factor→variable messages and the data; a leave-one-out message is the sum of the variable's
 * other messages, never a difference), work after every schedule, are exact on forests at a fixed point and give the Bethe factor
 * beliefs elsewhere.  One wave per factor on the f64 matrix cores: OUT is eliminated first, IN's marginal follows, and
 * the statistics are formed in residual coordinates directly (K = M^-1 Λ_out A), so that a flat OUT leaf gives Cov(r) = Q to rounding.
 * A factor with a NaN input record or datum is undefined; one whose inputs are defined and one of whose two factorisations meets a
 * non-positive pivot is not positive definite: its belief row is NaN, in the statistics it is counted in counts4[2] / counts4[3] and
 * its group's row is NaN (n_g excepted).
 * Grouping of cx_factor_statistics_mfma: factor_ids == NULL (and groups == NULL; n is ignored): one group per parameter set, every
 * two-variable CX_FACTOR_GAUSS_LINEAR factor counts, n_groups must exceed the largest set in use, and a factor of any other kind but
 * an opaque message is CX_ERR_UNSUPPORTED (naming it).  factor_ids, groups (length n): cx_factor_statistics' rules — one parameter set
 * per group and a factor listed twice CX_ERR_INVALID_ARGUMENT, an unknown id CX_ERR_NOT_FOUND, a factor of another kind
 * CX_ERR_UNSUPPORTED, group -1 skips.
 * Sums: the factors sorted by group, then factor index, are cut into partials of ceil(factors / W) factors of one group, W = 1024 at an
 * internal dim of 64 and 2048 below; one wave adds a partial's factors in order, a second kernel a group's partials in order; plain
 * f64, no atomics.  The cut depends on the grouping alone: two calls on one state of one handle are bit-identical (another handle
 * holding the same factors among others may cut elsewhere).  The lists of the last grouping are cached (an O(n) comparison on the host
 * for the same arrays) and rebuilt when other variables are observed; new rule parameters re-upload the A table only.
 * Device workspace: at most W wave workspaces of 6 KD^2 + 4 KD doubles (KD the internal dim) and one row of 2d + 3d^2 doubles per
 * partial, at most W + n_groups of them — at most 305 MB plus n_groups rows of 99,328 B at KD = d = 64 (1024 x 198,656 B of wave
 * workspaces, 1024 x 99,328 B of rows), 154 MB at 32, 39 MB at 16, whatever the number of factors.
 * cx_factor_beliefs_mfma works through its list W factors at a time.
 * Refused as cx_log_evidence_mfma refuses, each text naming the function: other families, a handle created with dim 1 - 4 (use
 * cx_factor_beliefs / cx_factor_statistics), partitioned handles CX_ERR_UNSUPPORTED; no graph, a captured stream, rule tables not on
 * the device CX_ERR_STATE; NULL arguments CX_ERR_INVALID_ARGUMENT.  cx_factor_beliefs and cx_factor_statistics keep refusing these
 * dims.  Synchronous; they move no message, marginal, readiness bit or counter. */
int32_t cx_factor_beliefs_mfma(cx_handle *h, int64_t n, const int64_t *factor_ids, double *out);
int32_t cx_factor_statistics_mfma(cx_handle *h, int64_t n, const int64_t *factor_ids, const int64_t *groups, int64_t n_groups, double *out,
                                  int64_t *counts4);

/* ---- smoothed disturbances at the matrix-core dims (added after ABI 9; no counterpart in the reference) ----
 * cx_factor_disturbances_mfma / cx_factor_disturbance_rows_mfma: for a handle created with dim 5 .. 64, the posterior of every factor's own
 * noise.  Every two-variable CX_FACTOR_GAUSS_LINEAR factor is x_out = A x_in + b + w, w ~ N(0, Q) (b: cx_set_factor_offsets_mfma, 0 unless
 * set), and r = x_out - A x_in - b IS w: the call returns, PER FACTOR, what cx_factor_statistics_mfma adds up per group — the disturbance
 * smoother of a state-space model (auxiliary residuals: outliers on the likelihood factors, structural breaks on the transitions).
 * A ROW is such a factor with either, both or none of its ends observed (what cx_factor_beliefs_mfma covers); opaque messages are part
 * of each variable's sum.  factor_ids == NULL returns every row in ascending factor id (cx_factor_disturbance_rows_mfma names them;
 * n is ignored; a factor of any other kind but an opaque message is CX_ERR_UNSUPPORTED, naming it), otherwise the n named factors in
 * the caller's order (an id may repeat): an unknown id is CX_ERR_NOT_FOUND, an opaque factor or one of another kind CX_ERR_UNSUPPORTED
 * (naming it).
 * out (may be NULL): n rows of d + d^2 doubles, d the CALLER's dim (an embedded dim returns the real block only),
 *     E[r | data][d] | Cov(r | data)[d][d] (row-major, full; symmetric to the rounding of its last product).
 * scores (may be NULL): n rows of two doubles,  t = E[r'Q^-1 r | data]  and  q = E[r]'Q^-1 E[r].  The kernel forms
 * s = sum_ab (Q^-1)_ab Cov(r)_ab and q separately over the real block and stores t = s + q, so t >= q whenever Cov(r) is positive
 * semi-definite to rounding; Q^-1 is the rule table's own.  t is the factor's share of -2 x the quadratic part of the EM Q-function and
 * what a reweighting scheme reads.
 * *total (may be NULL): the sum of t over the finite rows, folded 256 rows at a time in index order (no atomics).
 * counts4 = {rows, finite, undefined, not positive definite} with cx_factor_statistics_mfma's two rules: a NaN input record or datum
 * makes a row undefined, a failed pivot of either factorisation not positive definite; such a row is all NaN in out and in scores.
 * With both ends observed r is a number: the mean is y_out - A y_in - b, the covariance exact zeros and t = q.  Behind a flat OUT leaf
 * Cov(r) = Q to the rounding of one inverse, the mean is 0 and t = d: the factor says nothing about its disturbance.
 * The arithmetic is cx_factor_statistics_mfma's, on the f64 matrix cores; at most W waves per launch (W = 1024 at an
 * internal dim of 64, 2048 below), each with a workspace of its own and a contiguous run of rows.  A row's bits depend on neither the
 * wave that took it nor the other rows of the list: two calls on one state are bit-identical, rows, scores and total; the scores and
 * the total with out == NULL are the ones with rows; one factor alone gives the bits it gives in any list.  The payload passes through a
 * device buffer of at most 32 MiB, a launch and a copy per chunk with nothing waiting in between; scores and statuses are whole-call
 * arrays (25 bytes per row).  The row list of the last request is cached (an O(n) comparison on the host) and rebuilt when other
 * variables are observed.  It shares the factor records, the A table and the wave workspaces with the two calls above; calling it
 * between two cx_factor_statistics_mfma calls leaves the second one's output bit-identical to the first.
 * Refused as cx_factor_statistics_mfma refuses, each text naming the function: other families, a handle created with dim 1 - 4 (there
 * cx_factor_statistics sums the same moments per group), partitioned handles CX_ERR_UNSUPPORTED; no graph, a captured stream, a
 * parameter set never set CX_ERR_STATE; a NULL counts4 or n < 0 with ids CX_ERR_INVALID_ARGUMENT.  Synchronous; moves no message,
 * marginal, readiness bit or counter.  MI355X: profiles/factor_disturbances_mfma.md. */
int32_t cx_factor_disturbances_mfma(cx_handle *h, int64_t n, const int64_t *factor_ids, double *out, double *scores, double *total,
                                    int64_t *counts4);
int32_t cx_factor_disturbance_rows_mfma(cx_handle *h, int64_t cap, int64_t *factor_ids, int64_t *n_rows);

/* ---- predictive scores of the data at the matrix-core dims (added after ABI 9; no counterpart in the reference) ----
 * cx_predictive_mfma / cx_predictive_rows_mfma: cx_predictive and cx_predictive_rows for a handle created with dim 5 .. 64 — the same
 * contract, modes (CX_PREDICT_LOO, CX_PREDICT_CAUSAL), row order, row layout, counts4 = {rows, scored, undefined, improper}, NaN rule and
 * total (see there and DESIGN.md §4h), with d the CALLER's dim: a row of `out` is d + d^2 + 2 doubles,
 *     y^[d] | S[d][d] (row-major, full and symmetric) | log_density | maha.
 * A dim embedded in the next tile size (5 .. 15 in 16, 17 .. 31 in 32, 33 .. 63 in 64, or one forced by CX_MFMA_DIM) returns the real
 * block only, with the real model's values at any internal tile size.
 * A ROW at these dims is a two-variable CX_FACTOR_GAUSS_LINEAR factor  y = A x + N(0, Q)  whose CX_ROLE_OUT end is observed and whose
 * CX_ROLE_IN end is not: the likelihood factors of a state-space model, and the transition into a clamped state.  A datum on the
 * CX_ROLE_IN end stays out of scope, as at dim 1 - 4.  Opaque messages are part of a variable's sums.  factor_ids == NULL scores every
 * row in ascending factor id (cx_predictive_rows_mfma names them), otherwise the n named factors in the caller's order: an unknown id is
 * CX_ERR_NOT_FOUND, a factor that is not a row CX_ERR_UNSUPPORTED (naming it).
 * One wave per row on the f64 matrix cores, nothing a difference of messages: the cavity is the SUM of the stored
 * messages into x that the mode keeps (LOO: all but the row's own; CAUSAL: also none from a rule factor on which x is the CX_ROLE_IN end),
 * Λc = U'U, Z = U^-T A', S = Q + Z'Z, y^ = Z' U^-T ηc, then S = Us'Us for the score; log-determinant and quadratic form over the real
 * block.  A row is undefined when a stored message into x (kept or not) or the datum holds NaN; otherwise improper when nothing is kept
 * (flat by structure, such as the first observation of a chain without a prior under CX_PREDICT_CAUSAL), when a pivot of Λc or S is not
 * positive and finite, or when a pivot of Λc is at or below 64 d ulp of the same diagonal entry of the sum of ALL stored messages into x
 * (a message that carries no information — the one behind a leading gap, or a forecast's end — is stored as the rounding of a
 * difference, of either sign: it must not pass for a cavity).  A row that is not scored is all NaN.
 * *total (may be NULL): the sum of log_density over the scored rows, folded 256 rows at a time in index order (no atomics): two calls on
 * one state are bit-identical, rows and total, and the total with out == NULL is bit-identical to the one with rows.  The payload is
 * large (33,296 B per row at d = 64): it passes through a device buffer of at most 32 MiB, launched and copied a chunk at a time.
 * The rows of the last (mode, factor_ids) are cached (an O(n) comparison on the host for the same request) and rebuilt when the graph or
 * the observed flags change; the [A' | Q] table follows cx_set_factor_matrices.  MI355X: profiles/predictive_mfma.md.
 * cx_predictive and cx_predictive_rows keep returning CX_ERR_UNSUPPORTED at these dims exactly as before.
 * Refused as cx_log_evidence_mfma refuses, each text naming the function: other families, a handle created with dim 1 - 4 (use
 * cx_predictive), partitioned handles, a factor of another kind CX_ERR_UNSUPPORTED; no graph, a captured stream, rule tables not on the
 * device CX_ERR_STATE; an unknown mode, a NULL counts4 or n < 0 with ids CX_ERR_INVALID_ARGUMENT.  Synchronous; moves no message,
 * marginal, readiness bit or counter. */
int32_t cx_predictive_mfma(cx_handle *h, int32_t mode, int64_t n, const int64_t *factor_ids, double *out, double *total, int64_t *counts4);
int32_t cx_predictive_rows_mfma(cx_handle *h, int64_t cap, int64_t *factor_ids, int64_t *n_rows);

/* ---- causal marginals of the states at the matrix-core dims (added after ABI 9; no counterpart in the reference) ----
 * cx_causal_marginals_mfma: cx_causal_marginals for a handle created with dim 5 .. 64 — the same contract, modes (CX_CAUSAL_PREDICTED
 * with lag 0, CX_CAUSAL_FILTERED with lag >= 0), row order (variable_ids == NULL: every variable in ascending id, n ignored; otherwise
 * the n named variables in the caller's order), counts4 = {rows, finite, undefined, improper} and NaN rule (see there and DESIGN.md
 * §4j), with d the CALLER's dim: a row of `out` is d + d^2 doubles, mean[d] | cov[d][d] (row-major, full, symmetric to the last bit).
 * An observed variable's row is its datum and a zero covariance (one without a connection has no stored datum: its row is NaN and counted
 * undefined, as cx_causal_marginals returns it; cx_graph_create makes no such variable).  A dim embedded in the next tile size (5 .. 15 in 16, 17 .. 31 in 32,
 * 33 .. 63 in 64, or one forced by CX_MFMA_DIM) returns the real block only, with the real model's values at any internal tile size.
 * The classes are cx_causal_marginals', restricted to what these dims hold (two-variable CX_FACTOR_GAUSS_LINEAR factors and opaque
 * messages; a factor of another kind is CX_ERR_UNSUPPORTED, naming it) — cx_predictive_mfma's conventions, so that the two calls agree:
 *   U_i  opaque messages, and messages from factors on which i is the CX_ROLE_OUT end
 *   O_i  messages from factors on which i is the CX_ROLE_IN end and whose OUT end is observed
 *   T_i  messages from factors on which i is the CX_ROLE_IN end and whose OUT end is not observed
 *   predicted = Σ U_i,   filtered = Σ U_i + Σ O_i,   lag L = Σ U_i + Σ O_i + Σ_{a in T_i} β_a^(L),
 * β_a^(0) flat, β_a^(s) = the factor's own sum-product rule towards i applied to Σ O_j + Σ_{a' in T_j} β_a'^(s-1), j the OUT end of a:
 * sums of the messages kept, never the belief minus something.
 * One wave per item on the f64 matrix cores.  The backward pass is launched L times, one wave per T entry,
 * double-buffered over β (no launch reads what it writes): the wave-per-message rule of the sweeps on the sending slot's tables, with
 * j's O messages and the previous β of j's T entries as its sources.  An entry that no datum can have reached after s steps (the host
 * plan knows its distance to the nearest datum downstream) stores β^(s) as exact zeros — the rule would leave the rounding of a
 * difference, a "precision" of either sign — so a state behind the last datum returns the same bits at every lag; where the rule meets
 * a NaN input or a matrix that is not positive definite, β is NaN and every row that sums it is undefined.  The output kernel sums the
 * kept records of a row in ascending neighbour order, Λ = U'U, cov = (U^-T)'(U^-T), mean = (U^-T)' U^-T η.  A row is undefined when a
 * stored message into i (kept or not) or a summed β holds NaN; otherwise improper when nothing is kept, when a pivot is not positive and
 * finite, or when a pivot is at or below 64 d ulp of the same diagonal entry of the sum of ALL stored messages into i
 * (cx_predictive_mfma's flat-pivot rule: a message that carries no information is stored as the rounding of a difference, and alone in
 * the predicted sum — the state behind a leading gap — it must not pass for a prediction).  Statuses are folded 256 rows at a time in
 * index order (no atomics): two calls on one state are bit-identical, and a variable's numbers do not depend on which others share the
 * call.  The payload passes through a device buffer of at most 32 MiB, launched and copied a chunk at a time.
 * Cost: one wave per row; a lag L adds L launches over EVERY transition with two free ends, whatever rows are asked for.
 * Device workspace: with lag > 0, (1 for lag 1, otherwise 2) x (T entries) x (KD + KD²) doubles for β, KD the internal dim — 33,280 B
 * per entry and buffer at KD = 64: 6.7 GB for both at 1e5 transitions, 2.1 GB at KD = 32, 0.44 GB at KD = 16; allocated by the first
 * call with a lag and kept, growing only, until the handle's graph goes — also across a change of the observed flags, which rebuilds
 * the lists alone (a failed allocation is CX_ERR_OUT_OF_MEMORY); plus one record per variable with more than three sources.
 * The rows of the last (mode, lag > 0 or not, variable_ids) and the T entries are cached (an O(n) comparison on the host for the same
 * request) and rebuilt when the observed flags change; rule tables, messages and data are read by every call.  MI355X:
 * profiles/causal_marginals_mfma.md.  cx_causal_marginals keeps returning CX_ERR_UNSUPPORTED at these dims exactly as before.
 * Refused as cx_predictive_mfma refuses, each text naming the function: other families, a handle created with dim 1 - 4 (use
 * cx_causal_marginals), partitioned handles, a factor of another kind (a guard: cx_graph_create admits none at these dims) CX_ERR_UNSUPPORTED; no graph, a
 * captured stream, parameter sets never set CX_ERR_STATE; an unknown mode, lag < 0, lag > 0 with CX_CAUSAL_PREDICTED, a NULL out or counts4, or n < 0 with ids
 * CX_ERR_INVALID_ARGUMENT; an unknown id CX_ERR_NOT_FOUND.  Synchronous; moves no message, marginal, readiness bit or counter. */
int32_t cx_causal_marginals_mfma(cx_handle *h, int32_t mode, int32_t lag, int64_t n, const int64_t *variable_ids, double *out, int64_t *counts4);

/* ---- joint posterior samples at the matrix-core dims (added after ABI 9; no counterpart in the reference) ----
 * cx_sample_posterior_mfma: cx_sample_posterior for a handle created with dim 5 .. 64 — the same arguments, output layout, counts4 and
 * NaN rule (see "joint posterior samples" above), with d the CALLER's dim: out is a host array [n_samples][n][d] for variable_ids in the
 * caller's order (NULL: every variable in ascending id; n ignored), an observed variable's rows hold its datum (one on no connection has
 * no stored datum: NaN), counts4 = {free variables sampled, components, components with an undefined input, components not positive
 * definite}; every row of a failed component is NaN and the other components are unaffected.
 * noise != NULL: the caller's ε, a host array [n_samples][n_variables][d] in ascending variable-id order (rows of observed variables are
 * ignored); the call is then a fixed affine map of ε.  noise == NULL: Philox4x32-10 with the counter and key of cx_sample_posterior:
 * counter (j, v, s mod 2^32, s / 2^32), key (seed mod 2^32, seed / 2^32) yields components 2j and 2j + 1 of the variable of index v in
 * sample s; for an odd d the second normal of the last pair is dropped.  A dim embedded in the next tile size (5 .. 15 in 16, 17 .. 31 in
 * 32, 33 .. 63 in 64, or one forced by CX_MFMA_DIM) draws ε for the d real components only: the padding components get exactly zero
 * noise, stay exactly zero and are not returned.  A draw depends only on (seed, sample index, variable, component) and on the handle's
 * state: not on n_samples, on variable_ids or on how the call is chunked.  No atomics: two calls on one state are bit-identical.
 * The draw is §4g's q(x) = b_r(x_r) Π_a b_a(x_C | x_p) on the forest of non-observed variables, rooted where the tree
 * schedule's plan roots it.  Only two-variable CX_FACTOR_GAUSS_LINEAR factors and opaque messages exist at these dims.  For a link
 * factor with child end C and parent end p, (P, B') the rule table towards p:  M = P + Σ (C's other stored messages) = U'U,
 * x_C = M^-1 (B' x_p + Σ their η) + U^-1 ε_C;  the root: Λ_r = Σ all its stored messages = U'U, x_r = Λ_r^-1 η_r + U^-1 ε_r.  The
 * recursion is uncentred.  It reads the stored factor→variable messages and the data, never the marginals; at a fixed point on a
 * forest q is exactly p(x | data).  One wave per root and link computes the links on the f64 matrix cores, once per call; the samples
 * run in panels of 16 through a blocked scan of the affine maps (tiles of 64 items; CX_SAMPLE_MFMA_TILE = 2 .. 64, read when the plan is
 * built, sets another tile), in chunks of whole panels that keep the per-call scratch under 2^27 doubles (CX_SAMPLE_MFMA_CHUNK, a
 * multiple of 16 read per call, sets the samples per chunk); the least chunk is one panel.
 * A component is "not positive definite" when a pivot below d of a root's or a link's M is not positive and finite — and, decided on the
 * host, when the component touches no observed variable and carries no opaque message: it has no information at all, its stored messages
 * are roundings of differences, and it is not sampled (its rows are NaN, it counts under counts4[3]).  A component whose only
 * information is an opaque message that is itself flat is outside this contract: what it returns is not defined.
 * Device workspace: 2 KD² + KD doubles per non-observed variable for the links (G' | U^-T | off), KD the internal dim — 65,664 B at
 * KD = 64: 6.6 GB at 1e5 states, 1.6 GB at KD = 32, 0.41 GB at KD = 16; allocated with the plan and kept, growing only, until the
 * handle's graph goes, also across a change of the observed flags, which rebuilds the plan alone (a failed allocation is
 * CX_ERR_OUT_OF_MEMORY).  The plan is cached and rebuilt when the graph or the observed flags change; rule tables, messages and data are
 * read by every call.  cx_sample_posterior keeps returning CX_ERR_UNSUPPORTED at these dims exactly as before.
 * Refused as cx_causal_marginals_mfma refuses, each text naming the function: other families, a handle created with dim 1 - 4 (use
 * cx_sample_posterior), partitioned handles, a factor of another kind, a cycle among the non-observed variables (naming a variable of
 * the component) CX_ERR_UNSUPPORTED; no graph, a captured stream, parameter sets never set CX_ERR_STATE; n_samples < 1, a NULL out or
 * counts4, or n < 0 with ids CX_ERR_INVALID_ARGUMENT; an unknown id CX_ERR_NOT_FOUND.  Synchronous; moves no message, marginal,
 * readiness bit or counter. */
int32_t cx_sample_posterior_mfma(cx_handle *h, int64_t n_samples, uint64_t seed, const double *noise, int64_t n, const int64_t *variable_ids,
                                 double *out, int64_t *counts4);

/* ---- exact moments of linear functionals at the matrix-core dims (added after ABI 9; no counterpart in the reference) ----
 * cx_linear_moments_mfma: cx_linear_moments for a handle created with dim 5 .. 64 — the same arguments (see "linear functionals"
 * above), with d the CALLER's dim: the functionals in CSR form, weights [nnz][d]; a variable named twice in a functional counts with
 * the sum of its weights (merged on the host, in the order given); an observed variable adds w'·datum to the mean and nothing to cov.
 * mean is a host array [K]; cov is NULL (means only: the leaf-to-root scan is skipped) or a host array [K][K], one triangle computed
 * and mirrored; counts4 = {components, failed components, functionals made NaN, non-observed variables}.
 * The distribution is cx_sample_posterior_mfma's q(x) (above) on the forest of non-observed variables, rooted where that
 * call roots it, read from the stored factor→variable messages and the data, never from the marginals.  With x = x⁰ + B ε the sampler's
 * affine map: mean[k] = φ_k(x⁰) and cov = W B B' W'  — exact at a fixed point on a forest, elsewhere the moments of the q
 * the sampler draws from.  The recursion is uncentred, like the sampler's: §4r's note on data far from the origin applies unchanged.
 * A functional has a NaN mean and a NaN row and column of cov when it touches a failed component: one with a NaN input record, with a
 * pivot below d of a root's or a link's M that is not positive and finite, or with no information at all (decided on the host, as for
 * the sampler).  The other functionals are unaffected.
 * No atomics; every sum runs in a fixed order that does not depend on K: two calls on one state are bit-identical, a functional alone
 * gives the bits it gives among the others, and a call cut into chunks gives the bits of one chunk.
 * The call shares the sampler's plan and link workspace (whichever runs first builds them; the size is stated above) and computes the
 * links once per call.  Functionals run in panels of 16, in chunks of whole panels that keep the per-chunk scratch under 2^27 doubles
 * (CX_FN_MFMA_CHUNK, a multiple of 16 read per call, sets the functionals per chunk); the least chunk is one panel.  With cov, the noise
 * coordinates of all K functionals are kept ([non-observed variables][K in whole panels][KD] doubles): past 2^30 doubles, or block
 * partials of the covariance past 2^28 pairs, the call returns CX_ERR_OUT_OF_MEMORY; cov == NULL has no such bound.
 * CX_SAMPLE_MFMA_TILE and CX_MFMA_DIM act as for cx_sample_posterior_mfma.  cx_linear_moments keeps returning CX_ERR_UNSUPPORTED at
 * these dims exactly as before.
 * Refused as cx_sample_posterior_mfma refuses, each text starting with this function's name: other families, a handle created with dim
 * 1 - 4 (use cx_linear_moments), partitioned handles, a factor of another kind, a cycle among the non-observed variables
 * CX_ERR_UNSUPPORTED; no graph, a captured stream, parameter sets never set CX_ERR_STATE; n_functionals < 0 or above 32768, NULL offsets,
 * mean or counts4, NULL ids or weights with entries, offsets that do not start at 0 or that decrease CX_ERR_INVALID_ARGUMENT; an unknown
 * id CX_ERR_NOT_FOUND.  A refused call writes nothing.  Synchronous; moves no message, marginal, readiness bit or counter. */
int32_t cx_linear_moments_mfma(cx_handle *h, int64_t n_functionals, const int64_t *offsets, const int64_t *variable_ids, const double *weights,
                               double *mean, double *cov, int64_t *counts4);

/* ---- checkpoint (the reference keeps no persistent state — src/ has no serialisation at all) ----
 * The mutable state of a handle (every message buffer, the marginals, the observed-variable flags, the sweep counter)
 * as one relocatable host blob.  A blob restores only into a handle created with the same dim / family / schedule and
 * the same graph AND the same rule parameters (a fingerprint of the flattened graph, the factor parameters and the (A, Q) sets is
 * checked: a blob continues under the parameters it was exported with, or not at all; blobs of an earlier format are refused with
 * a version error); after cx_state_import the handle continues exactly
 * where the exporting one stood: the following sweeps reproduce its results bit for bit.  Halo buffers are not part
 * of the state (the next partitioned sweep exchanges them again).  Variational handles export their marginals and observed
 * flags (the structured family also the inner chain handle's state, inside the same blob). */
int32_t cx_state_bytes(const cx_handle *h, int64_t *bytes);
int32_t cx_state_export(cx_handle *h, void *buf, int64_t bytes);        /* synchronises the handle's stream */
int32_t cx_state_import(cx_handle *h, const void *buf, int64_t bytes);  /* validates everything before writing */

/* ---- measurement ------------------------------------------------------------------------------ */
#define CX_KERNEL_VAR_TO_FACTOR 0
#define CX_KERNEL_FACTOR_TO_VAR 1
#define CX_KERNEL_FUSED 2
#define CX_KERNEL_BATCH 3
#define CX_KERNEL_BIG_VAR 4
#define CX_KERNEL_HALO_BEGIN 5
#define CX_KERNEL_HALO_END 6
/* 7: unused since ABI 4 (was the two-sweeps-per-launch kernel) */
#define CX_KERNEL_COUNT 8
/* hipEvent pairs around kernel launches on the handle's stream: on == 1 every launch, on == n > 1 every n-th
 * launch of each kernel (events are barrier packets; a stride keeps the other launches back to back), 0 off */
int32_t cx_profile_enable(cx_handle *h, int32_t on);
int32_t cx_profile_read(cx_handle *h, int32_t kernel, double *total_ms, int64_t *launches); /* syncs; resets */
const char *cx_kernel_name(int32_t kernel);

#ifdef __cplusplus
}
#endif
#endif /* CORTEX_HIP_H */
