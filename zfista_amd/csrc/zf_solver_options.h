// zf_solver_options.h - the options of a margins solver as one record, and the one rule table that says which of them exist
// together.  Plain C++: no HIP include, no device pointer is read (tests/cpp/solver_options_host.cpp compiles it with g++ alone).
//
// A new loss or penalty is registered HERE: a field of zf_solver_options, an enumerator of zf_option, a row of ZF_OPTION_RULES
// (its kinds, its accept modes, the options it excludes - once per pair, in either row), and - for a loss - a line of
// zf_options_loss.  The extern "C" setter in zf_solver.hip is then the null check, zf_option_check, the allocation the option
// needs and zf_option_store; zf_desc_args (the evaluation entries) asks the same predicates
// about loss, response count and storage form (zf_loss_storage_exists and its three parts).
#pragma once
#include <float.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/zfista_hip.h"

constexpr int ZF_OPT_MAX_K = 16;   // responses (zf_kernels_mr.h: ZF_MR_MAX_K; zf_kernels_spmm.h: ZF_SPMM_MAX_K - asserted equal in zf_solver.hip)

// ---- the record ---------------------------------------------------------------------------------------------------------------
enum zf_option { ZF_OPT_L2, ZF_OPT_PF, ZF_OPT_HUBER, ZF_OPT_POISSON, ZF_OPT_MULTINOMIAL, ZF_OPT_ROWW, ZF_OPT_A32, ZF_OPT_K, ZF_OPT_COUNT };

struct zf_solver_options {
    double l2 = 0.0;               // elastic net (zf_solver_set_l2): g = lam |x|_1 + (l2 / 2) |x|^2; 0: every path is the l1 one
    const double* pf = nullptr;    // per-column penalty factors (zf_solver_set_penalty_factors; borrowed as b is): g = lam sum p_j |x_j|
    double huber = 0.0;            // Huber's loss (zf_solver_set_huber): delta > 0; 0: the squared loss
    bool poisson = false;          // the Poisson loss (zf_solver_set_poisson)
    bool multinomial = false;      // the multinomial loss on K responses (zf_solver_set_multinomial)
    const double* roww = nullptr;  // per-row sample weights (zf_solver_set_row_weights; borrowed as b is)
    const float* A32 = nullptr;    // the dense matrix stored in fp32 (zf_solver_set_matrix_f32; borrowed as desc.A is, which nothing reads then)
    int K = 1;                     // responses (zf_solver_set_responses, zf_solver_create_sparse_responses): desc holds the flattened lengths
};

// what zf_solver_create* fixed
struct zf_options_base {
    int kind;          // ZF_PROBLEM_*
    int world;
    int accept_mode;   // ZF_ACCEPT_*
    bool started;      // zf_solver_enqueue_init or zf_solver_restore has run
    int64_t m_rows, n; // the flattened lengths of the descriptor
    const void* b;
    bool small_shape;  // dense least squares of a shape, alignment and environment that the fused small-matrix kernels take - and no option has taken it off them since
    bool mfma_shape;   // dense, n % 32 == 0 and ZF_GEMV_MFMA not 0: the fp64 column sweep of one response runs on MFMA
};

// the argument of a setter call (the fields its option does not take stay 0)
struct zf_option_arg {
    double value;      // l2, delta
    const void* ptr;   // the factors, the weights, the fp32 matrix
    int K;
};

static inline bool zf_option_present(const zf_solver_options& o, int opt) {
    switch (opt) {
    case ZF_OPT_L2: return o.l2 > 0.0;   // (an explicit l2 = 0 is "not set")
    case ZF_OPT_PF: return o.pf != nullptr;
    case ZF_OPT_HUBER: return o.huber > 0.0;
    case ZF_OPT_POISSON: return o.poisson;
    case ZF_OPT_MULTINOMIAL: return o.multinomial;
    case ZF_OPT_ROWW: return o.roww != nullptr;
    case ZF_OPT_A32: return o.A32 != nullptr;
    case ZF_OPT_K: return o.K > 1;
    }
    return false;
}

static inline void zf_option_store(zf_solver_options* o, int opt, const zf_option_arg& a) {
    switch (opt) {
    case ZF_OPT_L2: o->l2 = a.value; break;
    case ZF_OPT_PF: o->pf = static_cast<const double*>(a.ptr); break;
    case ZF_OPT_HUBER: o->huber = a.value; break;
    case ZF_OPT_POISSON: o->poisson = true; break;
    case ZF_OPT_MULTINOMIAL: o->multinomial = true; break;
    case ZF_OPT_ROWW: o->roww = static_cast<const double*>(a.ptr); break;
    case ZF_OPT_A32: o->A32 = static_cast<const float*>(a.ptr); break;
    case ZF_OPT_K: o->K = a.K; break;
    }
}

// ---- which loss, response count and storage form exist together: the solver's rule table and zf_desc_args both ask here ---------
// K > 1 only with a loss whose rows kernels take K responses
static inline bool zf_loss_takes_responses(int loss) { return loss == ZF_LOSS_SQUARE || loss == ZF_LOSS_LOGISTIC || loss == ZF_LOSS_MULTINOMIAL; }
// the multinomial loss couples K >= 2 responses of a row, and the K-response sweeps read an fp64 A
static inline bool zf_multinomial_fits(int K, bool f32) { return K >= 2 && !f32; }
// no K-response sweep of a matrix stored in fp32
static inline bool zf_responses_fit_storage(int K, bool f32) { return !(K > 1 && f32); }
static inline bool zf_loss_storage_exists(int loss, int K, bool f32) {
    return (K == 1 || zf_loss_takes_responses(loss)) && (loss != ZF_LOSS_MULTINOMIAL || zf_multinomial_fits(K, f32)) && zf_responses_fit_storage(K, f32);
}

// ---- derived facts, each written once -------------------------------------------------------------------------------------------
static inline bool zf_kind_is_logistic(int kind) { return kind == ZF_PROBLEM_LOGISTIC_L1 || kind == ZF_PROBLEM_SPARSE_LOGISTIC_L1; }
// the ZF_LOSS_* code of a solver: the one place that reads the problem kind and the three loss options for it
static inline int zf_options_loss(int kind, const zf_solver_options& o) {
    return zf_kind_is_logistic(kind) ? (int)ZF_LOSS_LOGISTIC
           : o.huber > 0.0           ? (int)ZF_LOSS_HUBER
           : o.poisson               ? (int)ZF_LOSS_POISSON
           : o.multinomial           ? (int)ZF_LOSS_MULTINOMIAL
                                     : (int)ZF_LOSS_SQUARE;
}
// the dense least-squares kind holds the chunk sums of the loss kernels (as the dense logistic kind does from creation): every
// loss but the unweighted squared one writes them, and so do the wide residual kernels of K responses
static inline bool zf_options_need_loss_part(const zf_options_base& B, const zf_solver_options& o) {
    return B.kind == ZF_PROBLEM_LEAST_SQUARES_L1 && (o.huber > 0.0 || o.poisson || o.multinomial || o.roww || o.K > 1);
}
// the fused small-matrix kernels hold the unweighted squared loss of one response, the unfactored l1 step and an fp64 A: the
// path is open while the shape was eligible at creation and no option is set (the setters keep B.small_shape at this verdict, so a
// path once left stays left when l2 goes back to 0)
static inline bool zf_options_small_open(const zf_options_base& B, const zf_solver_options& o) {
    if (!B.small_shape) return false;
    for (int opt = 0; opt < ZF_OPT_COUNT; ++opt)
        if (zf_option_present(o, opt)) return false;
    return true;
}
// the elastic-net kernels leave g itself in the sum where the l1 kernels leave |x|_1 (or sum p |x|): the finalisation of a trial
// and of the initial point then scale it by 1 for lam
static inline bool zf_options_g_is_whole(const zf_solver_options& o) { return o.l2 > 0.0; }
// the matrix as the two sweeps see it: K responses are K columns on the matrix's own m x n; fp32 and K responses have no MFMA form
struct zf_options_view {
    int64_t m, n;
    int K;
    bool f32, mfma;
};
static inline zf_options_view zf_options_view_of(const zf_options_base& B, const zf_solver_options& o) {
    return zf_options_view{B.m_rows / o.K, B.n / o.K, o.K, o.A32 != nullptr, B.mfma_shape && !o.A32 && o.K == 1};
}

// ---- the rule table: one row per option ------------------------------------------------------------------------------------------
enum {   // argument checks
    ZF_ARG_FINITE_GE0 = 1,   // value finite and >= 0
    ZF_ARG_FINITE_GT0 = 2,   // value finite and > 0
    ZF_ARG_PTR = 4,          // ptr not NULL
    ZF_ARG_ALIGN16 = 32,     // ... and 16-byte aligned
    ZF_ARG_K = 8,            // K in 2 .. ZF_OPT_MAX_K, dividing m_rows and n
    ZF_ARG_B16 = 16,         // the solver's b 16-byte aligned
};
constexpr unsigned zf_kind_bit(int kind) { return 1u << kind; }
constexpr unsigned ZF_KINDS_LS = zf_kind_bit(ZF_PROBLEM_LEAST_SQUARES_L1) | zf_kind_bit(ZF_PROBLEM_SPARSE_LS_L1);
constexpr unsigned ZF_KINDS_DENSE = zf_kind_bit(ZF_PROBLEM_LEAST_SQUARES_L1) | zf_kind_bit(ZF_PROBLEM_LOGISTIC_L1);
constexpr unsigned ZF_KINDS_MARGINS = ZF_KINDS_LS | ZF_KINDS_DENSE | zf_kind_bit(ZF_PROBLEM_SPARSE_LOGISTIC_L1);
constexpr unsigned zf_opt_bit(int opt) { return 1u << opt; }

struct zf_option_rule {
    const char* entry;           // the extern "C" setter
    const char* noun;            // the option in another setter's refusal: "not with <noun>", "the solver already has <noun>"
    unsigned kinds;              // the kinds it admits ...
    const char* kinds_text;      // ... as the refusal lists them
    const char* no_remainder;    // why not with ZF_ACCEPT_REMAINDER; NULL: composes
    const char* no_resolved;     // why not with ZF_ACCEPT_RESOLVED; NULL: composes
    unsigned excludes;           // options that cannot be present with it: each unordered pair stands in ONE of its two rows
    bool once;                   // a second call is refused (false: it replaces the value)
    const char* needs;           // refusal when zf_loss_storage_exists says no to the record with this option added; NULL: nothing to need
    unsigned args;               // ZF_ARG_*
    const char* arg_name;        // what the argument is called in a refusal
    int started_code;            // after init / restore
};

#define ZF_NOT_THE_REMAINDER "scale |A (x+ - y)|^2 is not the Taylor remainder of this loss"
#define ZF_NOT_RESOLVED "the element-wise difference f(x+) - f(y) exists for the separable problem only"
static const zf_option_rule ZF_OPTION_RULES[ZF_OPT_COUNT] = {
    /* ZF_OPT_L2 */ {"zf_solver_set_l2", "l2 > 0 (zf_solver_set_l2)", ZF_KINDS_MARGINS,
                     "ZF_PROBLEM_LEAST_SQUARES_L1, ZF_PROBLEM_SPARSE_LS_L1, ZF_PROBLEM_LOGISTIC_L1 and ZF_PROBLEM_SPARSE_LOGISTIC_L1", nullptr, nullptr,
                     zf_opt_bit(ZF_OPT_PF) /* the ridge term would need the factors too */, false, nullptr, ZF_ARG_FINITE_GE0, "l2", ZF_ERR_STATE},
    /* ZF_OPT_PF */ {"zf_solver_set_penalty_factors", "penalty factors (zf_solver_set_penalty_factors)", ZF_KINDS_MARGINS,
                     "ZF_PROBLEM_LEAST_SQUARES_L1, ZF_PROBLEM_SPARSE_LS_L1, ZF_PROBLEM_LOGISTIC_L1 and ZF_PROBLEM_SPARSE_LOGISTIC_L1", nullptr, nullptr, 0,
                     false, nullptr, ZF_ARG_PTR | ZF_ARG_ALIGN16, "the factors", ZF_ERR_STATE},
    /* ZF_OPT_HUBER */ {"zf_solver_set_huber", "Huber's loss (zf_solver_set_huber)", ZF_KINDS_LS, "ZF_PROBLEM_LEAST_SQUARES_L1 and ZF_PROBLEM_SPARSE_LS_L1",
                        ZF_NOT_THE_REMAINDER, nullptr, zf_opt_bit(ZF_OPT_POISSON) | zf_opt_bit(ZF_OPT_MULTINOMIAL) | zf_opt_bit(ZF_OPT_K), false, nullptr,
                        ZF_ARG_FINITE_GT0, "delta", ZF_ERR_STATE},
    /* ZF_OPT_POISSON */ {"zf_solver_set_poisson", "the Poisson loss (zf_solver_set_poisson)", ZF_KINDS_LS,
                          "ZF_PROBLEM_LEAST_SQUARES_L1 and ZF_PROBLEM_SPARSE_LS_L1", ZF_NOT_THE_REMAINDER, ZF_NOT_RESOLVED,
                          zf_opt_bit(ZF_OPT_MULTINOMIAL) | zf_opt_bit(ZF_OPT_K), false, nullptr, 0, nullptr, ZF_ERR_STATE},
    /* ZF_OPT_MULTINOMIAL */ {"zf_solver_set_multinomial", "the multinomial loss (zf_solver_set_multinomial)", ZF_KINDS_LS,
                              "ZF_PROBLEM_LEAST_SQUARES_L1 and ZF_PROBLEM_SPARSE_LS_L1", ZF_NOT_THE_REMAINDER, ZF_NOT_RESOLVED, 0, true,
                              "the solver has no responses yet - a dense solver (its matrix in fp64) calls zf_solver_set_responses (K >= 2) BEFORE this "
                              "setter, a sparse one comes from zf_solver_create_sparse_responses",
                              ZF_ARG_B16, "b (the rows of Y)", ZF_ERR_STATE},
    /* ZF_OPT_ROWW */ {"zf_solver_set_row_weights", "row weights (zf_solver_set_row_weights)", ZF_KINDS_MARGINS,
                       "ZF_PROBLEM_LEAST_SQUARES_L1, ZF_PROBLEM_SPARSE_LS_L1, ZF_PROBLEM_LOGISTIC_L1 and ZF_PROBLEM_SPARSE_LOGISTIC_L1",
                       "the residual kernels that form scale |A (x+ - y)|^2 carry no weights", ZF_NOT_RESOLVED, 0, false, nullptr,
                       ZF_ARG_PTR, "the weights", ZF_ERR_STATE},
    /* ZF_OPT_A32 */ {"zf_solver_set_matrix_f32", "a matrix stored in fp32 (zf_solver_set_matrix_f32)", ZF_KINDS_DENSE,
                      "ZF_PROBLEM_LEAST_SQUARES_L1 and ZF_PROBLEM_LOGISTIC_L1", nullptr, nullptr, zf_opt_bit(ZF_OPT_K) /* the K-response sweeps read an fp64 A */,
                      false, nullptr, ZF_ARG_PTR | ZF_ARG_ALIGN16, "the matrix", ZF_ERR_ARG /* (as it always answered) */},
    /* ZF_OPT_K */ {"zf_solver_set_responses", "several responses (zf_solver_set_responses)", ZF_KINDS_DENSE,
                    "ZF_PROBLEM_LEAST_SQUARES_L1 and ZF_PROBLEM_LOGISTIC_L1", "the wide residual kernels of K dense responses form no remainder",
                    ZF_NOT_RESOLVED, 0, true, nullptr, ZF_ARG_K, "K", ZF_ERR_STATE},
};
#undef ZF_NOT_THE_REMAINDER
#undef ZF_NOT_RESOLVED

static inline bool zf_options_exclude(int a, int b) {
    return ((ZF_OPTION_RULES[a].excludes >> b) & 1u) || ((ZF_OPTION_RULES[b].excludes >> a) & 1u);
}

// May option `opt` with argument `a` be added to base B and record o?  ZF_OK, or ZF_ERR_ARG / ZF_ERR_STATE with the refusal in
// msg.  Reads only; the caller stores (zf_option_store) after whatever the option has to allocate.
static inline int zf_option_check(const zf_options_base& B, const zf_solver_options& o, int opt, const zf_option_arg& a, char* msg, size_t cap) {
    const zf_option_rule& R = ZF_OPTION_RULES[opt];
#define ZF_REFUSE(code, ...)             \
    do {                                 \
        snprintf(msg, cap, __VA_ARGS__); \
        return code;                     \
    } while (0)
    if ((R.args & ZF_ARG_PTR) && !a.ptr) ZF_REFUSE(ZF_ERR_ARG, "%s: null argument", R.entry);
    if (B.started) ZF_REFUSE(R.started_code, "%s: call after zf_solver_create and before zf_solver_enqueue_init / zf_solver_restore", R.entry);
    if (B.kind < 0 || B.kind >= 32 || !((R.kinds >> B.kind) & 1u)) ZF_REFUSE(ZF_ERR_ARG, "%s: only for %s", R.entry, R.kinds_text);
    if (B.world != 1) ZF_REFUSE(ZF_ERR_ARG, "%s: not for a sharded solve (world > 1)", R.entry);
    if ((R.args & ZF_ARG_FINITE_GE0) && !(a.value >= 0.0 && a.value <= DBL_MAX)) ZF_REFUSE(ZF_ERR_ARG, "%s: %s must be finite and >= 0", R.entry, R.arg_name);
    if ((R.args & ZF_ARG_FINITE_GT0) && !(a.value > 0.0 && a.value <= DBL_MAX)) ZF_REFUSE(ZF_ERR_ARG, "%s: %s must be finite and > 0", R.entry, R.arg_name);
    if ((R.args & ZF_ARG_ALIGN16) && (reinterpret_cast<uintptr_t>(a.ptr) & 15u))
        ZF_REFUSE(ZF_ERR_ARG, "%s: %s must be 16-byte aligned", R.entry, R.arg_name);
    if ((R.args & ZF_ARG_K) && !(a.K >= 2 && a.K <= ZF_OPT_MAX_K)) ZF_REFUSE(ZF_ERR_ARG, "%s: K must be 2 .. %d", R.entry, ZF_OPT_MAX_K);
    if (R.once && zf_option_present(o, opt)) ZF_REFUSE(ZF_ERR_ARG, "%s: the solver already has %s", R.entry, R.noun);
    if ((R.args & ZF_ARG_K) && !(B.m_rows % a.K == 0 && B.n % a.K == 0))
        ZF_REFUSE(ZF_ERR_ARG, "%s: m_rows and n of the solver must be multiples of K (they are m K and n K)", R.entry);
    if (B.accept_mode == ZF_ACCEPT_REMAINDER && R.no_remainder) ZF_REFUSE(ZF_ERR_ARG, "%s: not with ZF_ACCEPT_REMAINDER (%s)", R.entry, R.no_remainder);
    if (B.accept_mode == ZF_ACCEPT_RESOLVED && R.no_resolved) ZF_REFUSE(ZF_ERR_ARG, "%s: not with ZF_ACCEPT_RESOLVED (%s)", R.entry, R.no_resolved);
    zf_solver_options next = o;
    zf_option_store(&next, opt, a);
    if (zf_option_present(next, opt))   // (l2 = 0 adds nothing: it is accepted beside whatever is there)
        for (int other = 0; other < ZF_OPT_COUNT; ++other)
            if (other != opt && zf_option_present(o, other) && zf_options_exclude(opt, other))
                ZF_REFUSE(ZF_ERR_ARG, "%s: not with %s", R.entry, ZF_OPTION_RULES[other].noun);
    // (what the pairs above leave is a loss, a response count and a storage form that the evaluation entries know too)
    if (!zf_loss_storage_exists(zf_options_loss(B.kind, next), next.K, next.A32 != nullptr))
        ZF_REFUSE(ZF_ERR_ARG, "%s: %s", R.entry, R.needs ? R.needs : "no kernels for this loss, response count and storage form together");
    if ((R.args & ZF_ARG_B16) && (reinterpret_cast<uintptr_t>(B.b) & 15u)) ZF_REFUSE(ZF_ERR_ARG, "%s: %s must be 16-byte aligned", R.entry, R.arg_name);
#undef ZF_REFUSE
    return ZF_OK;
}
