// Host-only stand-in for the option setters of zf_solver.hip: csrc/zf_solver_options.h compiled with g++ alone
// (tests/test_solver_options_cpp.py builds a shared object from this file).
//
//   solver_options_apply   "apply this option to this base and record": zf_option_check, then zf_option_store when it says ZF_OK -
//                          what zf_solver_set_option does around its allocations.  The record lives in the caller's buffer.
//   solver_options_verdict the shared predicates on (loss, K, fp32): bit 0 zf_loss_takes_responses, 1 zf_multinomial_fits,
//                          2 zf_responses_fit_storage, 3 zf_loss_storage_exists.
//
// With -DSOLVER_OPTIONS_MAIN: a program that replays sequences from a text file, one per line -
//   kind world accept started m_rows n b K0 small ncalls { opt value ptr K rc small_after }*
// - and exits 1 at the first return code or small-matrix verdict that differs.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "../../zfista_amd/csrc/zf_solver_options.h"

// record: a buffer of at least 64 bytes (static_assert below), initialised by the first call of a sequence (K0 > 1: the K of
// zf_solver_create_sparse_responses).  small_shape: whether the path was open before the call; small_out: whether the fused
// small-matrix path is open after it (the next call's small_shape, as zf_solver_set_option keeps it).
extern "C" int solver_options_apply(int kind, int world, int accept_mode, int started, int64_t m_rows, int64_t n, uint64_t b, int small_shape,
                                    int K0, void* record, int first, int opt, double value, uint64_t ptr, int K, char* msg, int cap,
                                    int* small_out) {
    static_assert(sizeof(zf_solver_options) <= 64, "the callers' buffer");
    zf_solver_options* o = static_cast<zf_solver_options*>(record);
    if (first) {
        *o = zf_solver_options();
        if (K0 > 1) o->K = K0;
    }
    const zf_options_base B = {kind, world, accept_mode, started != 0, m_rows, n, reinterpret_cast<const void*>(b), small_shape != 0, false};
    const zf_option_arg a = {value, reinterpret_cast<const void*>(ptr), K};
    const zf_solver_options before = *o;
    const int rc = zf_option_check(B, *o, opt, a, msg, (size_t)cap);
    if (memcmp(&before, o, sizeof(before)) != 0) return -100;   // (the check reads only)
    if (rc == ZF_OK) zf_option_store(o, opt, a);
    *small_out = zf_options_small_open(B, *o) ? 1 : 0;
    return rc;
}

extern "C" int solver_options_verdict(int loss, int K, int f32) {
    return (zf_loss_takes_responses(loss) ? 1 : 0) | (zf_multinomial_fits(K, f32 != 0) ? 2 : 0) | (zf_responses_fit_storage(K, f32 != 0) ? 4 : 0) |
           (zf_loss_storage_exists(loss, K, f32 != 0) ? 8 : 0);
}

#ifdef SOLVER_OPTIONS_MAIN
int main(int argc, char** argv) {
    if (argc < 2) return 2;
    FILE* f = fopen(argv[1], "r");
    if (!f) return 2;
    long lines = 0, calls = 0;
    int kind, world, accept, started, K0, small, ncalls;
    long long m_rows, n;
    unsigned long long b;
    while (fscanf(f, "%d %d %d %d %lld %lld %llu %d %d %d", &kind, &world, &accept, &started, &m_rows, &n, &b, &K0, &small, &ncalls) == 10) {
        zf_solver_options rec;
        for (int c = 0; c < ncalls; ++c) {
            int opt, K, rc_want, small_want, small_got = -1;
            char value_text[64];
            unsigned long long ptr;
            double value;
            if (fscanf(f, "%d %63s %llu %d %d %d", &opt, value_text, &ptr, &K, &rc_want, &small_want) != 6) return 2;
            sscanf(value_text, "%lf", &value);   // (reads inf and nan)
            char msg[400] = "";
            const int rc = solver_options_apply(kind, world, accept, started, m_rows, n, b, small, K0, &rec, c == 0, opt, value, ptr, K, msg,
                                                (int)sizeof(msg), &small_got);
            if (rc != rc_want || (small_want >= 0 && small_got != small_want)) {
                printf("line %ld call %d: rc %d (want %d), small %d (want %d): %s\n", lines + 1, c, rc, rc_want, small_got, small_want, msg);
                return 1;
            }
            small = small_got;
            calls += 1;
        }
        lines += 1;
    }
    fclose(f);
    printf("replayed %ld sequences, %ld calls\n", lines, calls);
    return lines > 0 ? 0 : 2;
}
#endif
