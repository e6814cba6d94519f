// ugp_query.hpp -- the host code every device query family shares ("what a query family is"): the state's base, the
// attach protocol, the "attach first" sentence and the stage timers.  Host only: no kernel is defined or instantiated here.
#pragma once
#include <hip/hip_runtime.h>

#include <new>
#include <string>
#include <vector>

#include "ugp_dense.hpp"

namespace ugp {

// UGP_OK, or `err` as UGP_ERR_HIP with the call's name in front.
inline int hip_rc(const char *who, hipError_t err) {
    return err == hipSuccess ? UGP_OK : set_error(UGP_ERR_HIP, std::string(who) + ": " + hipGetErrorString(err));
}

// What every family's state holds.  The members of a derived state (its device buffers) go before the stream does.
struct QueryBase {
    int device = 0;
    hipStream_t stream = nullptr;                      // non-blocking; every launch and copy of the family runs on it
    const DfsTables *T = nullptr;                      // the handle's
    const std::vector<uint32_t> *dfs2bfs = nullptr;    // the handle's
    QueryBase() = default;
    QueryBase(const QueryBase &) = delete;
    QueryBase &operator=(const QueryBase &) = delete;
    ~QueryBase() {
        if (!stream) return;
        (void)hipSetDevice(device);
        (void)hipStreamDestroy(stream);
    }
};

// The derived state's device buffers are freed before ~QueryBase runs, so the device is set here for them as well.
template <class State>
void query_free(State *s) {
    if (!s) return;
    (void)hipSetDevice(s->device);
    delete s;
}

// Declared in a build() behind the host arrays it uploads: on every way out, an error return included, the stream has read them
// before they go.
struct StreamDrain {
    hipStream_t stream;
    ~StreamDrain() { (void)hipStreamSynchronize(stream); }
};

// The attach of a family, `who` = "ugp_<family>_attach".  check(T) is host only and runs before any state exists; build(S) fills
// the new state on its stream and leaves nothing in flight that reads host memory.  Both return UGP_OK or the code of an error they
// have set.  A failed attach leaves *out and *tables as they were.
template <class State, class Check, class Build>
int query_attach(const char *who, const ugp_tree_desc *tree, const std::vector<uint32_t> &dfs2bfs, const std::vector<uint32_t> &bfs2dfs,
                 int device, int entry_bits, DfsTables **tables, State **out, Check check, Build build) {
    if (!out || !tables) return set_error(UGP_ERR_INVALID, "null argument");
    DfsTables *const before = *tables;
    State *S = nullptr;
    int rc = dfs_tables(tree, dfs2bfs, bfs2dfs, device, entry_bits, tables);
    try {
        if (!rc) rc = dfs_tables_same_arrays(**tables, tree, dfs2bfs, who);
        if (!rc) rc = check(static_cast<const DfsTables &>(**tables));
        if (!rc) {
            S = new State();
            S->device = device;
            S->T = *tables;
            S->dfs2bfs = &dfs2bfs;
            if (hipSetDevice(device) != hipSuccess || hipStreamCreateWithFlags(&S->stream, hipStreamNonBlocking) != hipSuccess)
                rc = set_error(UGP_ERR_HIP, std::string(who) + ": hipStreamCreate failed");
        }
        if (!rc) rc = build(S);
    } catch (const std::bad_alloc &) { rc = set_error(UGP_ERR_NOMEM, "out of host memory"); }
    if (rc) {
        if (S && S->stream) (void)hipStreamSynchronize(S->stream);
        query_free(S);
        if (!before && *tables) { dfs_tables_free(*tables); *tables = nullptr; }
        return rc;
    }
    query_free(*out);
    *out = S;
    return UGP_OK;
}
struct NoCheck { int operator()(const DfsTables &) const { return UGP_OK; } };

// UGP_OK when the family is attached, else "<who>: no <family> tables: call ugp_<family>_attach first".
inline int query_ready(const void *S, const char *who, const char *family) {
    if (S) return UGP_OK;
    return set_error(UGP_ERR_INVALID, std::string(who) + ": no " + family + " tables: call ugp_" + family + "_attach first");
}

// Two events on one stream; lap() adds the milliseconds between start() and itself, once the stream has reached it.
struct EventPair {
    hipStream_t stream;
    hipEvent_t a = nullptr, b = nullptr;
    explicit EventPair(hipStream_t st) : stream(st) {}
    EventPair(const EventPair &) = delete;
    EventPair &operator=(const EventPair &) = delete;
    ~EventPair() { if (a) (void)hipEventDestroy(a); if (b) (void)hipEventDestroy(b); }
    hipError_t create() {
        const hipError_t e = hipEventCreate(&a);
        return e == hipSuccess ? hipEventCreate(&b) : e;
    }
    hipError_t start() { return hipEventRecord(a, stream); }
    hipError_t lap(double *acc) {
        float t = 0;
        hipError_t e = hipEventRecord(b, stream);
        if (e == hipSuccess) e = hipEventSynchronize(b);
        if (e == hipSuccess) e = hipEventElapsedTime(&t, a, b);
        *acc += t;
        return e;
    }
};

// One stage alone: an untimed run() (it sizes the workspaces), then *ms = the mean of `reps` runs back to back on `stream`.  run()
// returns UGP_OK or the code of an error it has set, which wins over a HIP error of the timer.
template <class F>
int timed(hipStream_t stream, const char *who, uint32_t reps, double *ms, F run) {
    EventPair ev(stream);
    hipError_t err = ev.create();
    int rc = err == hipSuccess ? run() : UGP_OK;
    if (!rc && err == hipSuccess) err = ev.start();
    for (uint32_t r = 0; r < reps && !rc && err == hipSuccess; r++) rc = run();
    double t = 0;
    if (!rc && err == hipSuccess) err = ev.lap(&t);
    (void)hipStreamSynchronize(stream);
    if (rc) return rc;
    if (err != hipSuccess) return hip_rc(who, err);
    *ms = t / reps;
    return UGP_OK;
}

}  // namespace ugp
