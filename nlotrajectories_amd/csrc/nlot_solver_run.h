// The host driver of the batched solve: the environment knobs, the per-call resources, the stream plan of one
// global step (launch_step) and run<DYN>(), which nlot_solve_batch (nlot_solve_api.hip) dispatches to.
// Included by nlot_solver.hip after the kernels it launches.
#pragma once
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "nlot_solver_ws.h"

namespace nlot {

// the statistics of the thread's last call and the sampled-timing period (defined in nlot_solve_api.hip)
extern thread_local NlotSolveStats g_stats;
extern int g_timing;  // nlot_set_timing: 0 off; k: one step in each group of k, at position (step / k) % k (rotating)

// like NLOT_HIP_CHECK for calls that return an NLOT_ERR_* code (set_error already holds their message)
#define NLOT_RC_CHECK(expr)                              \
    do {                                                 \
        if (const int rc_ = (expr)) return rc_;          \
    } while (0)

// Steps run ahead of the host: every kernel reads its step's active count on the device (cnt[2] of the
// step's counter set, written by the previous step's k_accept), and grids are sized by the host's last
// known count, an upper bound (the active set only shrinks).  The host waits once per KPIPE steps: it
// then learns the counts (the D2H copies of each step's counters land in a pinned ring) and whether any
// instance is still active; the at most KPIPE - 1 steps launched past the end exit at once.
constexpr int KPIPE = 8;

// The environment knobs of run(): A/B switches and diagnostics, read once per call (read_knobs, which holds the
// variable names and the clamps).  None of them changes the results.
struct RunKnobs {
    int setprio = 0;      // NLOT_SETPRIO: the side-stream chains raise their waves' issue priority (Ws::prio)
    int stream_prio = 0;  // NLOT_STREAM_PRIO: 1 restoration stream at the highest priority, 2 the correction stream too
    int soc_fork = 0;     // NLOT_SOC_FORK 0..2: corrections fork after k_iter_a / at the step's start / after the full MLP
    bool early_value = true;    // NLOT_EARLY_VALUE: the previous step's candidates evaluate on a fourth stream (+1.3 %, r04)
    bool mlp_reuse = true;      // NLOT_MLP_REUSE=0: the full MLP launch does not reuse the value launch's forward
    int spec_threshold = 8192;  // NLOT_SPEC_THRESHOLD: speculative backtracking (NSPEC step lengths) up to this many active
    int spec_bulk = 2;          // NLOT_SPEC_BULK 1..NSPEC: step lengths per later round above it (2: -1.5 % vs 1, r03 ab8)
    int ric_tries = 1;          // NLOT_RIC_TRIES >= 1: k_ric's inertia-correction attempts per launch ...
    int ric_tries_min = 0;      // NLOT_RIC_TRIES_MIN: ... while more than this many instances are active (r05az)
    bool resto_tries = true;    // NLOT_RESTO_TRIES: the same cap for the restoration solves; 0: every attempt in one launch
    double progress_s = 0;      // NLOT_PROGRESS=seconds: a line on stderr now and then (long continuous calls)
    int kpipe = KPIPE;          // NLOT_PIPE 1..KPIPE: steps between host synchronisations
    int resto_force = 0;        // NLOT_RESTO_BOUND >= 1 (test_resto_grid_bound_same_results): restoration grids of at most n
    bool step_kernel = true;    // NLOT_STEP_KERNEL: counter bookkeeping by k_step_end; 0: by the copies it replaces
    const char* step_log = nullptr;  // NLOT_STEP_LOG=path (scripts/step_trace.py): one line of counters per global step
};

// w: the learned SDF's weights or null; P: SDF points per instance
static RunKnobs read_knobs(const MlpDev* w, int64_t P) {
    RunKnobs k;
    // speculation while one value launch stays below ~56 GFLOP of forward work: 8192 instances of the metric
    // (P = 204 corners x 33,536 FLOP; measured best of {512, 2048, 8192} x {1, 2} at B = 65536), 138 of the
    // stress config (P = 1028 x 394,752 FLOP)
    if (w) {
        const double H = w->H, fwd = 2.0 * (2.0 * H + w->n_hidden * H * H + H);
        k.spec_threshold = (int)std::max(1.0, std::min(1e9, 5.6e10 / (fwd * (double)P)));
    }
    if (const char* e = getenv("NLOT_SETPRIO")) k.setprio = atoi(e);
    if (const char* e = getenv("NLOT_STREAM_PRIO")) k.stream_prio = atoi(e);
    if (const char* e = getenv("NLOT_SOC_FORK")) k.soc_fork = std::max(0, std::min(2, atoi(e)));
    if (const char* e = getenv("NLOT_EARLY_VALUE")) k.early_value = atoi(e) != 0;
    if (const char* e = getenv("NLOT_MLP_REUSE")) k.mlp_reuse = strcmp(e, "0") != 0;
    if (const char* e = getenv("NLOT_SPEC_THRESHOLD")) k.spec_threshold = atoi(e);
    if (const char* e = getenv("NLOT_SPEC_BULK")) k.spec_bulk = std::max(1, std::min(NSPEC, atoi(e)));
    if (const char* e = getenv("NLOT_RIC_TRIES")) k.ric_tries = std::max(1, atoi(e));
    if (const char* e = getenv("NLOT_RIC_TRIES_MIN")) k.ric_tries_min = atoi(e);
    if (const char* e = getenv("NLOT_RESTO_TRIES")) k.resto_tries = atoi(e) != 0;
    if (const char* e = getenv("NLOT_PROGRESS")) k.progress_s = atof(e);
    if (const char* e = getenv("NLOT_PIPE")) k.kpipe = std::max(1, std::min(KPIPE, atoi(e)));
    if (const char* e = getenv("NLOT_RESTO_BOUND")) k.resto_force = std::max(1, atoi(e));
    if (const char* e = getenv("NLOT_STEP_KERNEL")) k.step_kernel = atoi(e) != 0;
    k.step_log = getenv("NLOT_STEP_LOG");
    return k;
}

// host-side resources of one call, released on every return path (NLOT_HIP_CHECK returns early)
struct Res {
    int* hcnt = nullptr;            // the pinned counter ring: KPIPE steps x 2 sets, then the free-slot count and
    int* dcnt = nullptr;            // k_admit's error flag (read at every synchronisation); dcnt: its device address
    hipEvent_t ev[KPIPE][10] = {};  // [8], [9]: the early value launch (NLOT_EARLY_VALUE) on its stream
    hipEvent_t noev[10] = {};       // the untimed steps' (no events)
    bool timed[KPIPE] = {};         // the ring slot's step was timed
    hipStream_t s2 = nullptr, s3 = nullptr, s4 = nullptr;       // side streams: SOC / restoration / early values
    hipEvent_t e_a = nullptr, e_soc = nullptr, e_r = nullptr, e_s = nullptr, e_v0 = nullptr, e_v1 = nullptr;
    // the pinned ring, the side streams (NLOT_STREAM_PRIO), the fork / join events and, for a timed call, the ring's
    // timing events
    int create(int stream_prio, bool timing) {
        NLOT_HIP_CHECK(hipHostMalloc((void**)&hcnt, (KPIPE * 2 * CSET + 2) * sizeof(int),
                                     hipHostMallocMapped | hipHostMallocCoherent));
        if (stream_prio > 0) {
            int prio_least = 0, prio_greatest = 0;
            NLOT_HIP_CHECK(hipDeviceGetStreamPriorityRange(&prio_least, &prio_greatest));
            if (stream_prio >= 2) NLOT_HIP_CHECK(hipStreamCreateWithPriority(&s2, hipStreamNonBlocking, prio_greatest));
            else NLOT_HIP_CHECK(hipStreamCreateWithFlags(&s2, hipStreamNonBlocking));
            NLOT_HIP_CHECK(hipStreamCreateWithPriority(&s3, hipStreamNonBlocking, prio_greatest));
        } else {
            NLOT_HIP_CHECK(hipStreamCreateWithFlags(&s2, hipStreamNonBlocking));
            NLOT_HIP_CHECK(hipStreamCreateWithFlags(&s3, hipStreamNonBlocking));
        }
        for (hipEvent_t* e : {&e_a, &e_soc, &e_r, &e_s, &e_v0, &e_v1})
            NLOT_HIP_CHECK(hipEventCreateWithFlags(e, hipEventDisableTiming));
        NLOT_HIP_CHECK(hipStreamCreateWithFlags(&s4, hipStreamNonBlocking));
        if (timing)
            for (auto& r : ev)
                for (auto& e : r) NLOT_HIP_CHECK(hipEventCreate(&e));
        return NLOT_OK;
    }
    ~Res() {
        for (auto& r : ev)
            for (auto& e : r)
                if (e) (void)hipEventDestroy(e);
        for (hipEvent_t e : {e_a, e_soc, e_r, e_s, e_v0, e_v1})
            if (e) (void)hipEventDestroy(e);
        if (s2) (void)hipStreamDestroy(s2);
        if (s3) (void)hipStreamDestroy(s3);
        if (s4) (void)hipStreamDestroy(s4);
        if (hcnt) (void)hipHostFree(hcnt);
    }
};

// one call's state: what launch_step and the synchronisations between the windows share
struct RunCtx {
    // fixed for the call
    const NlotSolverOptions& o;
    const NlotMlp* mlp;  // null unless use_mlp
    hipStream_t st;
    RunKnobs kn;
    bool use_mlp = false;
    int64_t P = 0;                          // SDF points per instance
    int Bi = 0, capacity = 0, t_every = 0;  // instances; slots; g_timing at the start of the call
    Ws ws{};
    NlotProblem* dP = nullptr;  // the workspace header's device copies of the problem, the dimensions and ws
    Dims* dD = nullptr;
    Ws* dW = nullptr;
    Res res;
    MlpOut mo{}, mo_t[2] = {};  // outputs of the full launch and, by step parity, of the value launches
    MlpReuse reuse[2] = {};
    // progress
    int64_t step = 0, synced = 0;  // the step being launched; the first step not yet folded into the statistics
    int n_active = 0, cur = 0;     // the host's last known active count; which of ws.act is this step's list
    bool init_step = true;         // this step runs the INIT pass (step 0, and the step after an admission)
    int next_admit = 0;            // the first instance not yet admitted
    // grid bound of the restoration kernels (they read the exact list count on the device): every active instance
    // until a synchronisation shows how many are restoring (an instance enters at most one step before)
    int resto_bound = 0;
    std::vector<int> slog;  // the step log's rows (kn.step_log), 15 ints each

    template <int DYN>
    int launch_step();
    int sync_window();
    void fold(int64_t last);
    int admit(const double* x0, const double* xg, const double* Xinit);
};

// fold the counters of steps synced .. last into g_stats (after a synchronisation); updates n_active
inline void RunCtx::fold(int64_t last) {
    for (int64_t sj = synced; sj <= last; ++sj) {
        const int j = (int)(sj % kn.kpipe), qj = (int)(sj & 1);
        const int* hc = res.hcnt + 2 * CSET * j + CSET * qj;
        const int next_active = res.hcnt[2 * CSET * j + CSET * (qj ^ 1) + 2];
        if (kn.step_log) {
            // step, active, full-eval instances, trial slots, reused points, Newton solves, restoration count,
            // corrections, restoration solves, next active, the Newton solves' diagnostics
            slog.push_back((int)sj);
            slog.push_back(n_active);
            for (int i = 0; i < 8; ++i) slog.push_back(i == 2 ? 0 : hc[i]);
            slog.push_back(next_active);
            for (int i = 8; i < 11; ++i) slog.push_back(hc[i]);
            slog.push_back(hc[15]);
        }
        g_stats.iterations = (int)(sj + 1);
        if (use_mlp) {
            g_stats.mlp_points_full += (int64_t)hc[0] * P;
            g_stats.mlp_points_value += (int64_t)hc[1] * P;
            g_stats.mlp_points_full_reused += (int64_t)hc[3];
            g_stats.mlp_full_launches++;
            g_stats.mlp_value_launches++;
        }
        g_stats.ric_launches++;
        g_stats.ric_solves += hc[4];
        g_stats.ric_soc_solves += hc[6];
        g_stats.ric_resto_solves += hc[7];
        g_stats.filter_peak = std::max(g_stats.filter_peak, hc[11]);
        g_stats.filter_forgotten += hc[12];
        const hipEvent_t* e = res.ev[j];
        if (res.timed[j]) {
            g_stats.timed_steps++;
            g_stats.timed_ric_solves += hc[4];
            if (use_mlp) {
                g_stats.timed_points_full += (int64_t)hc[0] * P;
                g_stats.timed_points_value += (int64_t)hc[1] * P;
                g_stats.timed_points_full_reused += (int64_t)hc[3];
            }
        }
        if (res.timed[j] && use_mlp) {
            float a = 0, v = 0;
            (void)hipEventElapsedTime(&a, e[0], e[1]);
            (void)hipEventElapsedTime(&v, e[2], e[3]);
            g_stats.mlp_full_ms += a;
            g_stats.mlp_value_ms += v;
            if (kn.early_value) {
                float v0 = 0;
                (void)hipEventElapsedTime(&v0, e[8], e[9]);
                g_stats.mlp_value_ms += v0;
            }
        }
        if (res.timed[j]) {
            float a = 0, r = 0;
            (void)hipEventElapsedTime(&a, e[4], e[5]);
            (void)hipEventElapsedTime(&r, e[6], e[7]);
            g_stats.iterate_ms += a;
            g_stats.ric_ms += r;
        }
        n_active = next_active;
        if (n_active == 0) break;  // the later steps of this window found nothing to do
    }
    synced = last + 1;
}

// The launches of one global step, step, over the n_active instances of the list ws.act[cur].
// (launch_ric and soc_chain stay lambdas, in this order: the order in which a function template first names the
// kernel instantiations is their order in the code object.)
template <int DYN>
int RunCtx::launch_step() {
    const hipStream_t s2 = res.s2, s3 = res.s3, s4 = res.s4;
    const int ric_blocks_per = RicG<DYN>::IPW;
    const int* act = ws.act[cur];
    int* nxt = ws.act[cur ^ 1];
    const int* actr = ws.actr[cur];
    int* nxtr = ws.actr[cur ^ 1];
    const int kq = (int)(step % kn.kpipe);
    // one step in t_every, at a position in its group of t_every steps that rotates from group to group: the
    // host's synchronisations (and so admissions, INIT steps) fall at a fixed position of the KPIPE window, so a
    // fixed sampling phase would time one kind of step only
    res.timed[kq] = t_every > 0 && step % t_every == (step / t_every) % t_every;
    hipEvent_t* ev = res.timed[kq] ? res.ev[kq] : res.noev;
    // Point lists are appended to by the kernel that moves an instance into the phase needing them
    // (k_iter_b: first line-search round; k_accept: the new iterate, or the next round), so the lists
    // and counters of step s + 1 fill while step s runs: both alternate by step parity q.
    const int q = (int)(step & 1);
    int* C = ws.cnt + CSET * q;
    int* Cn = ws.cnt + CSET * (q ^ 1);
    if (!kn.step_kernel) NLOT_HIP_CHECK(hipMemsetAsync(Cn, 0, CSET * sizeof(int), st));
    // The second-order corrections (substitution, short) and the restoration instances' Newton solves (a longer
    // sequential sweep, few instances) touch disjoint instances from the main Newton solve: they run on a side
    // stream, forked after k_iter_a, so their latency hides under k_ric's; k_iter_b joins the corrections, the
    // value-MLP launch joins the restoration chain (k_resto_b appends to the same trial list).
    // the factorising Newton solves (main stream): the lane-group k_ric
    auto launch_ric = [&](const int* list, const int* count, int mode, int* diag, int tries) {
        hipLaunchKernelGGL((k_ric<DYN, false>), dim3((n_active + ric_blocks_per - 1) / ric_blocks_per), dim3(64), 0,
                           st, dP, dD, dW, list, n_active, count, mode, diag, tries);
    };
    // the second-order corrections' chain (k_iter_a's SOC pass: their stages; k_ric<DYN, false, true>: the
    // substitutions) needs no MLP evaluation: it forks to the side stream at the start of the step (soc_fork 1),
    // after the full MLP launch (2), or after the one k_iter_a launch that also does the evaluations (0)
    auto soc_chain = [&](bool with_pass) {
        NLOT_HIP_CHECK(hipEventRecord(res.e_s, st));
        NLOT_HIP_CHECK(hipStreamWaitEvent(s2, res.e_s, 0));
        if (with_pass)
            hipLaunchKernelGGL(k_iter_a<DYN>, dim3(n_active), dim3(64), 0, s2, dP, dD, o, dW, act, ws.x0s, ws.xgs,
                               (int)PASS_SOC, C, Cn);
        hipLaunchKernelGGL((k_ric<DYN, false, true>), dim3((n_active + ric_blocks_per - 1) / ric_blocks_per),
                           dim3(64), 0, s2, dP, dD, dW, ws.socl, n_active, C + 6, (int)MODE_NEWTON, nullptr, 1 << 30);
        NLOT_HIP_CHECK(hipEventRecord(res.e_soc, s2));
        return NLOT_OK;
    };
    if (kn.soc_fork == 1) NLOT_RC_CHECK(soc_chain(true));
    // the value launch's first part: the candidates the previous step's k_accept / k_resto_ls listed (ranks
    // [0, C[14]), C[14] = C[1] now) evaluate on a side stream while this step's evaluations and Newton solves run;
    // the second part (after k_iter_b) covers the candidates added since (ranks [C[14], C[1]))
    if (use_mlp && kn.early_value) {
        if (!kn.step_kernel) NLOT_HIP_CHECK(hipMemcpyAsync(C + 14, C + 1, sizeof(int), hipMemcpyDeviceToDevice, st));
        NLOT_HIP_CHECK(hipEventRecord(res.e_v0, st));
        NLOT_HIP_CHECK(hipStreamWaitEvent(s4, res.e_v0, 0));
        if (ev[0]) (void)hipEventRecord(ev[8], s4);
        const int rc = launch_mlp_strided(mlp->dev, ws.tpts[q], (int64_t)n_active * NSPEC, C + 14, (int)P, 0, nullptr,
                                          mo_t[q], false, s4);
        if (ev[0]) (void)hipEventRecord(ev[9], s4);
        NLOT_RC_CHECK(rc);
        NLOT_HIP_CHECK(hipEventRecord(res.e_v1, s4));
    }
    // speculative backtracking only while the GPU is latency-bound (few active instances); in the
    // throughput-bound bulk it would multiply the value-MLP work for the same accepted steps
    const int nspec = n_active > kn.spec_threshold ? kn.spec_bulk : NSPEC;
    if (use_mlp) {
        if (init_step) hipLaunchKernelGGL(k_points, dim3(n_active), dim3(64), 0, st, dP, dD, dW, act, C);
        if (ev[0]) (void)hipEventRecord(ev[0], st);
        // contiguous rank-major list: P_per = 1, count = (#instances) * P read on the device
        MlpReuse ru = reuse[q ^ 1];  // the previous step's trial list
        ru.nreused = C + 3;            // statistics: points whose forward was reused
        NLOT_RC_CHECK(launch_mlp_strided(mlp->dev, ws.pts, n_active, C + 0, (int)P, 0, nullptr, mo, true, st, &ru));
        if (ev[0]) (void)hipEventRecord(ev[1], st);
    }
    if (kn.soc_fork == 2) NLOT_RC_CHECK(soc_chain(true));
    if (ev[4]) (void)hipEventRecord(ev[4], st);
    // restoration phases (list actr, count C[5]) on a stream of their own, forked once the step's evaluations are
    // in (they need nothing else of the step; disjoint instances): k_resto_a, their Newton solves, k_resto_b.  An
    // instance k_resto_a returns to the original problem is passed by this step's k_iter_a and continues next
    // step (k_accept); round 5: k_resto_a (one long wavefront per restoring instance, ~0.5 ms) left the main
    // stream's critical path
    const int n_resto = std::min(n_active, resto_bound);
    if (n_resto > 0) {
        NLOT_HIP_CHECK(hipEventRecord(res.e_a, st));
        NLOT_HIP_CHECK(hipStreamWaitEvent(s3, res.e_a, 0));
        hipLaunchKernelGGL(k_resto_a<DYN>, dim3(n_resto), dim3(64), 0, s3, dP, dD, o, dW, actr, ws.x0s, ws.xgs, C);
        hipLaunchKernelGGL((k_ric<DYN, true>), dim3((n_resto + ric_blocks_per - 1) / ric_blocks_per), dim3(64), 0, s3,
                           dP, dD, dW, actr, n_resto, C + 5, (int)MODE_NEWTON, C + 15,
                           kn.resto_tries && n_active > kn.ric_tries_min ? kn.ric_tries : 1 << 30);
        hipLaunchKernelGGL(k_resto_b<DYN>, dim3(n_resto), dim3(64), 0, s3, dP, dD, o, dW, actr, C,
                           use_mlp ? ws.tpts[q] : nullptr);
        NLOT_HIP_CHECK(hipEventRecord(res.e_r, s3));
    }
    if (init_step) {  // INIT: slack push + least-squares multipliers (one Riccati solve)
        hipLaunchKernelGGL(k_iter_a<DYN>, dim3(n_active), dim3(64), 0, st, dP, dD, o, dW, act, ws.x0s, ws.xgs,
                           (int)PASS_INIT, C, Cn);
        launch_ric(act, C + 2, (int)MODE_LSQ, nullptr, 1 << 30);
    }
    hipLaunchKernelGGL(k_iter_a<DYN>, dim3(n_active), dim3(64), 0, st, dP, dD, o, dW, act, ws.x0s, ws.xgs,
                       (int)(kn.soc_fork == 0 ? PASS_ALL : PASS_EVAL), C, Cn);
    if (kn.soc_fork == 0) NLOT_RC_CHECK(soc_chain(false));
    // the Newton solves and the corrections run over the compacted lists k_iter_a wrote (ws.ricl / ws.socl,
    // counts C[4] / C[6]; the grids are host bounds, blocks past the count exit): one group per instance that
    // has work, so a launch holds as many wavefronts as it has solves / 4
    if (ev[6]) (void)hipEventRecord(ev[6], st);
    launch_ric(ws.ricl, C + 4, (int)MODE_NEWTON, C + 8, n_active > kn.ric_tries_min ? kn.ric_tries : 1 << 30);
    if (ev[6]) (void)hipEventRecord(ev[7], st);
    NLOT_HIP_CHECK(hipStreamWaitEvent(st, res.e_soc, 0));
    hipLaunchKernelGGL(k_iter_b<DYN>, dim3(n_active), dim3(64), 0, st, dP, dD, o, dW, act, C,
                       use_mlp ? ws.tpts[q] : nullptr, Cn);
    if (n_resto > 0) NLOT_HIP_CHECK(hipStreamWaitEvent(st, res.e_r, 0));
    if (ev[4]) (void)hipEventRecord(ev[5], st);
    if (use_mlp) {
        // the wait for the early part comes before the timing event: ev[2]..ev[3] is the second part's own time
        if (kn.early_value) NLOT_HIP_CHECK(hipStreamWaitEvent(st, res.e_v1, 0));
        if (ev[0]) (void)hipEventRecord(ev[2], st);
        MlpReuse vb{};
        vb.base = C + 14;
        NLOT_RC_CHECK(launch_mlp_strided(mlp->dev, ws.tpts[q], (int64_t)n_active * NSPEC, C + 1, (int)P, 0, nullptr,
                                         mo_t[q], false, st, kn.early_value ? &vb : nullptr));
        if (ev[0]) (void)hipEventRecord(ev[3], st);
    }
    // the next round's candidate count uses this step's nspec (n_active only shrinks: speculation
    // starts at most KPIPE steps late; the accepted alpha is the same either way)
    if (n_resto > 0)
        hipLaunchKernelGGL(k_resto_ls<DYN>, dim3(n_resto), dim3(64), 0, st, dP, dD, o, dW, actr, ws.x0s, ws.xgs, C, Cn,
                           use_mlp ? ws.tpts[q ^ 1] : nullptr, use_mlp ? ws.tval[q] : nullptr, nspec);
    hipLaunchKernelGGL(k_accept<DYN>, dim3(n_active), dim3(64), 0, st, dP, dD, o, dW, act, nxt, nxtr, ws.x0s, ws.xgs, C, Cn,
                       use_mlp ? ws.tpts[q ^ 1] : nullptr, use_mlp ? ws.tval[q] : nullptr, nspec);
    NLOT_HIP_CHECK(hipGetLastError());
    // this step's counters (C) and the next step's active count (Cn[2]), before step + 1 clears C
    if (kn.step_kernel) {
        hipLaunchKernelGGL(k_step_end, dim3(1), dim3(64), 0, st, ws.cnt, q, res.dcnt + 2 * CSET * kq,
                           res.dcnt + KPIPE * 2 * CSET);
    } else {
        NLOT_HIP_CHECK(hipMemcpyAsync(res.hcnt + 2 * CSET * kq, ws.cnt, 2 * CSET * sizeof(int),
                                      hipMemcpyDeviceToHost, st));
    }
    cur ^= 1;
    init_step = false;
    return NLOT_OK;
}

// The host's wait at the end of a window of kn.kpipe steps (step is the window's last): the error flag, the next
// windows' restoration grid bound, the statistics and the active count.
inline int RunCtx::sync_window() {
    int* hflag = res.hcnt + KPIPE * 2 * CSET;
    if (!kn.step_kernel)
        NLOT_HIP_CHECK(hipMemcpyAsync(hflag, ws.cnt + 2 * CSET, 2 * sizeof(int), hipMemcpyDeviceToHost, st));
    NLOT_HIP_CHECK(hipStreamSynchronize(st));
    if (hflag[1] != 0) {  // k_admit's shortfall or a list that outgrew its grid (grid_guard): fail now, not at the end
        set_error(grid_error(hflag[1]));
        return NLOT_ERR_INVALID;
    }
    // restoration lists of the window: the next launches' grid bound (their kernels read the exact count)
    const int kq = (int)(step % kn.kpipe);
    int rmax = 0;
    for (int j = 0; j <= kq; ++j) rmax = std::max(rmax, res.hcnt[2 * CSET * j + CSET * (((step - kq + j) & 1) ^ 1) + 5]);
    resto_bound = std::min(Bi, 2 * rmax + 256);
    if (kn.resto_force) resto_bound = std::min(resto_bound, kn.resto_force);
    fold(step);
    return NLOT_OK;
}

// Continuous batching (o.max_active = capacity < B): the first `capacity` instances start; whenever a host
// synchronisation finds at least capacity / 32 slots free, the next instances (index order) join the active
// list and run their INIT step (corners, slack push, least-squares multipliers) in the next step.  Every
// instance runs the same iteration sequence whenever it starts, so the results do not depend on capacity;
// what changes is that the latency-bound tail of one group overlaps the bulk of the next.
inline int RunCtx::admit(const double* x0, const double* xg, const double* Xinit) {
    if (next_admit >= Bi || (capacity - n_active < std::max(1, capacity / 32) && n_active != 0))
        return NLOT_OK;
    // instances next_admit .. next_admit + n_new - 1 take free slots (the free-slot count is capacity - the
    // next active count: every instance that left the list freed its slot), join the next step's active
    // list, and start (k_init_state on those slots)
    const int n_new = std::min(capacity - n_active, Bi - next_admit);
    int* Cadm = ws.cnt + CSET * ((step + 1) & 1);
    hipLaunchKernelGGL(k_admit, dim3(1), dim3(1024), 0, st, ws.act[cur], Cadm, ws.sinst, ws.freel,
                       ws.cnt + 2 * CSET, next_admit, n_new);
    hipLaunchKernelGGL(k_init_state, dim3(n_new), dim3(64), 0, st, dP, dD, o, ws, x0, xg, Xinit, ws.act[cur],
                       Cadm);
    NLOT_HIP_CHECK(hipGetLastError());
    next_admit += n_new;
    n_active += n_new;
    init_step = true;
    return NLOT_OK;
}

// NLOT_KPROF / NLOT_RIC_PROF builds: print the device-side phase timers of the call to stderr and clear them
static int dump_kprof(hipStream_t st) {
#ifdef NLOT_KPROF
    unsigned long long kp[4][16];
    NLOT_HIP_CHECK(hipStreamSynchronize(st));
    NLOT_HIP_CHECK(hipMemcpyFromSymbol(kp, HIP_SYMBOL(g_kprof), sizeof(kp)));
    const char* kn[4] = {"k_iter_a", "k_iter_b", "k_accept", "k_resto"};
    for (int k = 0; k < 4; ++k)
        if (kp[k][15]) {
            fprintf(stderr, "[kprof] %s waves %llu: us per wave", kn[k], kp[k][15]);
            for (int i = 0; i < 15; ++i)
                if (kp[k][i]) fprintf(stderr, " [%d] %.2f", i, kp[k][i] * 1e-2 / kp[k][15]);
            fprintf(stderr, "\n");
        }
    const unsigned long long z[4][16] = {};
    NLOT_HIP_CHECK(hipMemcpyToSymbol(HIP_SYMBOL(g_kprof), z, sizeof(z)));
#endif
    return NLOT_OK;
}
static int dump_ric_prof(hipStream_t st) {
#ifdef NLOT_RIC_PROF  // g_ric_prof: k_ric's sweeps by kind of solve
    unsigned long long hp[3][5];
    NLOT_HIP_CHECK(hipStreamSynchronize(st));
    NLOT_HIP_CHECK(hipMemcpyFromSymbol(hp, HIP_SYMBOL(g_ric_prof), sizeof(hp)));
    const char* kinds[3] = {"newton", "correction", "restoration"};
    for (int k = 0; k < 3; ++k)
        if (hp[k][4])
            fprintf(stderr, "[ric_prof] %s solves %llu: us per solve backward %.2f F1 %.2f F2 %.2f F3+mult %.2f\n",
                    kinds[k], hp[k][4], hp[k][0] * 1e-2 / hp[k][4], hp[k][1] * 1e-2 / hp[k][4],
                    hp[k][2] * 1e-2 / hp[k][4], hp[k][3] * 1e-2 / hp[k][4]);
    const unsigned long long z[3][5] = {};
    NLOT_HIP_CHECK(hipMemcpyToSymbol(HIP_SYMBOL(g_ric_prof), z, sizeof(z)));
#endif
    return NLOT_OK;
}

// NLOT_STEP_LOG: one line per global step appended to path (the rows fold() collected)
static void write_step_log(const char* path, const std::vector<int>& slog) {
    if (!path || slog.empty()) return;
    if (FILE* f = fopen(path, "a")) {
        for (size_t i = 0; i < slog.size(); i += 15) {
            for (int j = 0; j < 15; ++j) fprintf(f, j ? " %d" : "%d", slog[i + j]);
            fputc('\n', f);
        }
        fclose(f);
    }
}

template <int DYN>
int run(const NlotProblem& p, const NlotSolverOptions& o, const NlotMlp* mlp, const double* x0, const double* xg,
        const double* Xinit, double* X, double* U, double* S, double* cost, int32_t* status, int32_t* iters,
        int64_t B, void* workspace, hipStream_t st) {
    Dims dm = make_dims(p);
    dm.gcb = o.general_bounds ? 1 : 0;
    const bool use_mlp = p.sdf_kind == NLOT_SDF_MLP;
    const int64_t P = (int64_t)dm.ppk * (dm.N + 1);
    const int cap_slots = (int)slot_count(B, o.max_active);
    RunCtx c{o, mlp, st, read_knobs(use_mlp ? &mlp->dev : nullptr, P)};
    const RunKnobs& kn = c.kn;
    c.use_mlp = use_mlp;
    c.P = P;
    c.Bi = (int)B;
    c.capacity = c.next_admit = c.n_active = cap_slots;
    Ws& ws = c.ws;
    ws = carve(dm, cap_slots, use_mlp, workspace);
    ws.oX = X;
    ws.oU = U;
    ws.oS = S;
    ws.ocost = cost;
    ws.ostat = status;
    ws.oiters = iters;
    ws.prio = kn.setprio;
    c.dP = (NlotProblem*)((char*)workspace + kHdrProblem);
    c.dD = (Dims*)((char*)workspace + kHdrDims);
    c.dW = (Ws*)((char*)workspace + kHdrWs);
    static_assert(sizeof(NlotProblem) <= kHdrDims - kHdrProblem && sizeof(Dims) <= kHdrWs - kHdrDims &&
                  sizeof(Ws) <= kHdr - kHdrWs, "workspace header");
    NLOT_HIP_CHECK(hipMemcpyAsync(c.dP, &p, sizeof(NlotProblem), hipMemcpyHostToDevice, st));
    NLOT_HIP_CHECK(hipMemcpyAsync(c.dD, &dm, sizeof(Dims), hipMemcpyHostToDevice, st));
    NLOT_HIP_CHECK(hipMemcpyAsync(c.dW, &ws, sizeof(Ws), hipMemcpyHostToDevice, st));
    g_stats = NlotSolveStats{};
    g_stats.filter_capacity = FILT_MAX;
    g_stats.timing_every = c.t_every = g_timing;
    g_stats.slots_in_lds = 0;  // stage slots live in the HBM workspace; k_ric stages them through LDS
    hipLaunchKernelGGL(k_init_state, dim3(cap_slots), dim3(64), 0, st, c.dP, c.dD, o, ws, x0, xg, Xinit, nullptr, nullptr);
    NLOT_HIP_CHECK(hipGetLastError());
    Res& res = c.res;
    NLOT_RC_CHECK(res.create(kn.stream_prio, c.t_every != 0));
    if (use_mlp) {
        const int64_t plane = P * (int64_t)cap_slots * NSPEC;  // the MLP output planes hold the slots' points
        MlpOut& mo = c.mo;
        mo.val = ws.mo; mo.gx = ws.mo + plane; mo.gy = ws.mo + 2 * plane; mo.hxx = ws.mo + 3 * plane;
        mo.hxy = ws.mo + 4 * plane; mo.hyx = mo.hxy; mo.hyy = ws.mo + 5 * plane;
        mo.sv = mo.sg = mo.sh = 1;
        // trial lists (by step parity): values + ReLU patterns, reused by the next full launch at the
        // accepted point
        for (int q = 0; q < 2; ++q) {
            c.mo_t[q].val = ws.tval[q];
            c.mo_t[q].sv = 1;
            c.mo_t[q].mask = ws.tmask[q];
            c.mo_t[q].mask_plane = plane;
            c.reuse[q] = MlpReuse{kn.mlp_reuse ? ws.tsrc : nullptr, ws.tpts[q], ws.tval[q], ws.tmask[q], plane, nullptr};
        }
    }
    const auto t0 = std::chrono::steady_clock::now();  // NLOT_PROGRESS
    double t_prog = kn.progress_s;
    // a safety net against a phase-machine bug, not an iteration limit (max_iter bounds every instance): at most
    // 64 global steps per iteration per admission wave
    const int64_t waves = (B + cap_slots - 1) / cap_slots;
    const int64_t max_steps = ((int64_t)o.max_iter + 2) * 64 * (waves + 1);
    c.resto_bound = o.resto ? (kn.resto_force ? std::min(c.Bi, kn.resto_force) : c.Bi) : 0;
    NLOT_HIP_CHECK(hipMemsetAsync(ws.cnt, 0, 64 * sizeof(int), st));  // both sets, the free-slot count, error flag
    res.hcnt[0] = cap_slots;  // step 0's active count (cnt[2] of counter set 0)
    NLOT_HIP_CHECK(hipMemcpyAsync(ws.cnt + 2, res.hcnt, sizeof(int), hipMemcpyHostToDevice, st));
    NLOT_HIP_CHECK(hipStreamSynchronize(st));  // the pinned source is reused below
    NLOT_HIP_CHECK(hipHostGetDevicePointer((void**)&res.dcnt, res.hcnt, 0));
    for (c.step = 0; c.step < max_steps && c.n_active > 0; ++c.step) {
        NLOT_RC_CHECK(c.launch_step<DYN>());
        if (c.step % kn.kpipe != kn.kpipe - 1) continue;
        NLOT_RC_CHECK(c.sync_window());
        if (kn.progress_s > 0) {
            const double t = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
            if (t >= t_prog) {
                fprintf(stderr, "[nlot] %.0f s: step %lld, %d active, %d of %d instances admitted\n", t,
                        (long long)c.step, c.n_active, c.next_admit, c.Bi);
                fflush(stderr);
                t_prog = t + kn.progress_s;
            }
        }
        NLOT_RC_CHECK(c.admit(x0, xg, Xinit));
    }
    if (c.synced < c.step) {  // a window the loop left before its synchronisation point
        NLOT_HIP_CHECK(hipStreamSynchronize(st));
        c.fold(c.step - 1);
    }
    NLOT_RC_CHECK(dump_kprof(st));
    NLOT_RC_CHECK(dump_ric_prof(st));
    if (c.n_active > 0 || c.next_admit < c.Bi) {
        set_error("nlot_solve_batch: the global step cap was reached with instances unfinished (phase-machine bug)");
        return NLOT_ERR_INVALID;
    }
    write_step_log(kn.step_log, c.slog);
    // every instance wrote its outputs when it left the active list (k_accept -> retire)
    NLOT_HIP_CHECK(hipMemcpyAsync(res.hcnt, ws.cnt + 2 * CSET, 2 * sizeof(int), hipMemcpyDeviceToHost, st));
    NLOT_HIP_CHECK(hipStreamSynchronize(st));
    if (res.hcnt[1] != 0 || res.hcnt[0] != cap_slots) {
        set_error(res.hcnt[1] != 0 ? grid_error(res.hcnt[1])
                                   : "nlot_solve_batch: slot bookkeeping mismatch (free slots at the end != capacity)");
        return NLOT_ERR_INVALID;
    }
    return NLOT_OK;
}

}  // namespace nlot
