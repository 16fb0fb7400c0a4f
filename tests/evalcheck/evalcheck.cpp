// evalcheck.cpp -- TEST INFRASTRUCTURE.  Compiles the evaluation's rules (reinfocus_amd/csrc/rf_eval.h: targets, positions,
// the accumulation, the per-thread tree, the row and the best rule) for the host, with plain loops in place of the
// kernels' threads and arrays in place of the block's butterflies, so that a CPU-only test can compare the definition with
// the numpy twin (environments/evaluation.py) before any GPU sees it.  Never loaded by the product package.
#include <math.h>
#include <stdint.h>

#include <vector>

#include "../../reinfocus_amd/csrc/rf_eval.h"

using namespace rf;

namespace {

// eval_block_treesum: the 256 threads' values through the wave butterflies, the four wave results through the butterfly
// over four lanes, + 0.0
double block_treesum(std::vector<double> v)
{
    std::vector<double> next(kEvalThreads);
    for (int off = 1; off < 64; off <<= 1) {
        for (int t = 0; t < kEvalThreads; ++t)
            next[t] = v[t] + v[t ^ off];
        v = next;
    }
    double w[4] = {v[0], v[64], v[128], v[192]}, x[4];
    for (int off = 1; off < 4; off <<= 1) {
        for (int t = 0; t < 4; ++t)
            x[t] = w[t] + w[t ^ off];
        for (int t = 0; t < 4; ++t)
            w[t] = x[t];
    }
    return w[0] + 0.0;
}

template <typename Leaf>
double treesum(int E, Leaf leaf)
{
    const int leaves = eval_leaves(E);
    std::vector<double> v(kEvalThreads);
    for (int t = 0; t < kEvalThreads; ++t) {
        const int first = t * leaves;
        v[t] = eval_thread_tree(leaves, [&](int j) { return first + j < E ? leaf(first + j) : 0.0; });
    }
    return block_treesum(v);
}

} // namespace

extern "C" {

int evc_target(int m, int E, int i) { return eval_target(m, E, i); }
int evc_slots(int m, int E) { return eval_slots(m, E); }
int evc_first(int m, int E, int i) { return eval_first(m, E, i); }
int evc_leaves(int E) { return eval_leaves(E); }

void evc_locate(int m, int E, int p, int *lane_slot)
{
    eval_locate(m, E, p, lane_slot[0], lane_slot[1]);
}

// rf_eval_accumulate on host arrays
void evc_accumulate(int groups, int m, int E, const double *final_return, const int *final_length, int *counts,
                    double *returns, int *lengths)
{
    const int K = eval_slots(m, E);
    for (long long lane = 0; lane < (long long)groups * m; ++lane)
        eval_accumulate_one(eval_target(m, E, (int)(lane % m)), final_return[lane], final_length[lane], counts + lane,
                            returns + lane * K, lengths + lane * K);
}

// rf_eval_finish on host arrays
void evc_finish(int groups, int m, int E, unsigned long long serial, const int *counts, const double *returns,
                const int *lengths, double *results, double *best_mean, long long *best_serial, uint8_t *improved)
{
    const int K = eval_slots(m, E);
    for (int g = 0; g < groups; ++g) {
        const size_t base = (size_t)g * (size_t)m;
        long long kept = 0;
        for (int i = 0; i < m; ++i)
            kept += counts[base + i] > 0 ? counts[base + i] : 0;
        if (kept != E) {
            eval_write_row(results + (size_t)g * 8, false, 0.0, 0.0, false, 0, 0, 0.0, (int)kept, serial);
            improved[g] = 0;
            continue;
        }
        const double *mine = returns + base * K;
        const int *mine_lengths = lengths + base * K;
        auto at = [&](int p) {
            int i, k;
            eval_locate(m, E, p, i, k);
            return (size_t)i * (size_t)K + (size_t)k;
        };
        int64_t min_key = INT64_MAX, max_key = INT64_MIN;
        bool any_nan = false;
        for (int p = 0; p < E; ++p) {
            const double x = mine[at(p)];
            if (x != x) {
                any_nan = true;
                continue;
            }
            const int64_t key = eval_key(x);
            min_key = key < min_key ? key : min_key;
            max_key = key > max_key ? key : max_key;
        }
        const double N = (double)E;
        const double mean = treesum(E, [&](int p) { return mine[at(p)]; }) / N;
        const double std = sqrt(treesum(E, [&](int p) {
                                    const double d = mine[at(p)] - mean;
                                    return d * d;
                                }) / N);
        const double mean_length = treesum(E, [&](int p) { return (double)mine_lengths[at(p)]; }) / N;
        eval_write_row(results + (size_t)g * 8, true, mean, std, any_nan, min_key, max_key, mean_length, (int)kept, serial);
        eval_best(true, mean, serial, best_mean + g, best_serial + g, improved + g);
    }
}

} // extern "C"

#ifdef EVALCHECK_MAIN
#include <stdio.h>

// The stand-alone form (what a sanitizer build runs): every (m, E) of a small grid through the targets, the positions, an
// accumulation in which every lane ends every step, and the finish.
int main()
{
    for (int m = 1; m <= 11; ++m)
        for (int E : {1, 2, 5, 20, 257, 300}) {
            const int K = eval_slots(m, E), G = 2, n = G * m;
            int total = 0;
            for (int i = 0; i < m; ++i) {
                if (eval_first(m, E, i) != total)
                    return 1;
                total += eval_target(m, E, i);
            }
            if (total != E)
                return 2;
            for (int p = 0; p < E; ++p) {
                int at[2];
                evc_locate(m, E, p, at);
                if (at[1] < 0 || at[1] >= eval_target(m, E, at[0]) || eval_first(m, E, at[0]) + at[1] != p)
                    return 3;
            }
            std::vector<int> counts(n, 0), lengths((size_t)n * K, 0), final_length(n, 3);
            std::vector<double> returns((size_t)n * K, 0.0), final_return(n);
            for (int step = 0; step < K + 1; ++step) {
                for (int e = 0; e < n; ++e)
                    final_return[e] = 0.25 * e - step;
                evc_accumulate(G, m, E, final_return.data(), final_length.data(), counts.data(), returns.data(),
                               lengths.data());
            }
            std::vector<double> results((size_t)G * 8), best(G, -INFINITY);
            std::vector<long long> best_serial(G, 0);
            std::vector<uint8_t> improved(G, 7);
            evc_finish(G, m, E, 1, counts.data(), returns.data(), lengths.data(), results.data(), best.data(),
                       best_serial.data(), improved.data());
            for (int g = 0; g < G; ++g)
                if (results[(size_t)g * 8 + 5] != E || results[(size_t)g * 8 + 6] != 0.0 || improved[g] != 1 ||
                    results[(size_t)g * 8 + 4] != 3.0)
                    return 4;
        }
    printf("evalcheck ok\n");
    return 0;
}
#endif
