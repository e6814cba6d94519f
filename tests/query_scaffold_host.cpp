// A stand-alone host program around usher_amd/csrc/ugp_query.hpp (tests/test_query_scaffold_cpu.py builds and runs it): query_attach
// with a stub state whose build fails after the state exists, and timed with a run that fails in the warm-up alone.  The few HIP
// calls the header makes are defined here, so no device is needed, and the table functions of ugp_dense.cpp are stand-ins.
// Prints one line per check and exits with the number of failed ones.
#include <cstdio>
#include <string>
#include <vector>

#include "ugp_query.hpp"

static int g_streams = 0, g_stream_syncs = 0, g_events = 0, g_tables = 0;
static std::string g_error;

extern "C" {
hipError_t hipSetDevice(int) { return hipSuccess; }
hipError_t hipStreamCreateWithFlags(hipStream_t *s, unsigned) { g_streams++; *s = reinterpret_cast<hipStream_t>(&g_streams); return hipSuccess; }
hipError_t hipStreamSynchronize(hipStream_t) { g_stream_syncs++; return hipSuccess; }
hipError_t hipStreamDestroy(hipStream_t) { g_streams--; return hipSuccess; }
hipError_t hipEventCreate(hipEvent_t *e) { g_events++; *e = reinterpret_cast<hipEvent_t>(&g_events); return hipSuccess; }
hipError_t hipEventDestroy(hipEvent_t) { g_events--; return hipSuccess; }
hipError_t hipEventRecord(hipEvent_t, hipStream_t) { return hipSuccess; }
hipError_t hipEventSynchronize(hipEvent_t) { return hipSuccess; }
hipError_t hipEventElapsedTime(float *ms, hipEvent_t, hipEvent_t) { *ms = 6.0f; return hipSuccess; }
}

namespace ugp {
int set_error(int code, const std::string &msg) { g_error = msg; return code; }
int dfs_tables(const ugp_tree_desc *, const std::vector<uint32_t> &, const std::vector<uint32_t> &, int device, int, DfsTables **tables) {
    if (!*tables) { *tables = new DfsTables(); (*tables)->device = device; g_tables++; }
    return UGP_OK;
}
void dfs_tables_free(DfsTables *t) { if (t) { delete t; g_tables--; } }
int dfs_tables_same_arrays(const DfsTables &, const ugp_tree_desc *, const std::vector<uint32_t> &, const char *) { return UGP_OK; }
}  // namespace ugp

static int g_states = 0;
struct StubState : ugp::QueryBase {
    int tag = 0;
    StubState() { g_states++; }
    ~StubState() { g_states--; }
};

static int failed = 0;
static void expect(bool ok, const char *what) {
    std::printf("%s %s\n", ok ? "ok  " : "FAIL", what);
    std::fflush(stdout);
    failed += ok ? 0 : 1;
}

int main() {
    const std::vector<uint32_t> order{0};
    ugp_tree_desc tree{};
    ugp::DfsTables *tables = nullptr;
    StubState *state = nullptr;
    auto attach = [&](int tag, int check_rc, int build_rc) {
        return ugp::query_attach("ugp_stub_attach", &tree, order, order, 0, 31, &tables, &state,
                                 [&](const ugp::DfsTables &) { return check_rc; },
                                 [&](StubState *S) { S->tag = tag; return build_rc ? ugp::set_error(build_rc, "build failed") : UGP_OK; });
    };
    // a first attach whose build fails: no state, no stream, and the tables it made are gone
    expect(attach(1, 0, UGP_ERR_HIP) == UGP_ERR_HIP && g_error == "build failed", "a failing build returns its code and message");
    expect(state == nullptr && g_states == 0 && g_streams == 0, "a failed first attach leaves no state and no stream");
    expect(tables == nullptr && g_tables == 0, "a failed first attach frees the tables it made");
    // a good attach
    expect(attach(2, 0, 0) == UGP_OK && state && state->tag == 2 && state->T == tables && state->dfs2bfs == &order && state->stream,
           "a good attach stores a state with its stream, tables and order");
    expect(g_states == 1 && g_streams == 1 && g_tables == 1, "one state, one stream, one set of tables");
    // a second attach whose build fails after its state exists: the first state stays, the new one and its stream are gone
    ugp::DfsTables *const kept = tables;
    const int syncs = g_stream_syncs;
    expect(attach(3, 0, UGP_ERR_UNSUPPORTED) == UGP_ERR_UNSUPPORTED, "a failing build of a second attach returns its code");
    expect(state && state->tag == 2, "the handle keeps the state of the good attach");
    expect(g_states == 1 && g_streams == 1, "the new state and its stream are gone");
    expect(g_stream_syncs > syncs, "the new state's stream was synchronised before it went");
    expect(tables == kept && g_tables == 1, "tables that an earlier attach made stay");
    // a refused check makes no state at all
    expect(attach(4, UGP_ERR_INVALID, 0) == UGP_ERR_INVALID && state && state->tag == 2 && g_states == 1 && g_streams == 1, "a refused check leaves the handle alone");
    // a second good attach replaces the first
    expect(attach(5, 0, 0) == UGP_OK && state && state->tag == 5 && g_states == 1 && g_streams == 1, "a second good attach replaces the first state");

    if (!state) return failed + 100;   // nothing to time on
    // timed: the mean over reps; a run that fails only in the warm-up fails the call; the events are released on every path
    double ms = -1;
    int calls = 0;
    expect(ugp::timed(state->stream, "ugp_stub_time", 3, &ms, [&] { calls++; return (int)UGP_OK; }) == UGP_OK && calls == 4 && ms == 2.0,
           "timed runs once untimed, then reps times, and reports elapsed / reps");
    ms = -1; calls = 0;
    expect(ugp::timed(state->stream, "ugp_stub_time", 3, &ms, [&] { return calls++ ? (int)UGP_OK : ugp::set_error(UGP_ERR_INVALID, "warm-up failed"); }) == UGP_ERR_INVALID &&
               calls == 1 && ms == -1 && g_error == "warm-up failed",
           "a run that fails in the warm-up fails the call, runs no more and leaves *ms alone");
    ms = -1; calls = 0;
    expect(ugp::timed(state->stream, "ugp_stub_time", 3, &ms, [&] { return ++calls == 3 ? ugp::set_error(UGP_ERR_UNSUPPORTED, "rep failed") : (int)UGP_OK; }) == UGP_ERR_UNSUPPORTED &&
               calls == 3 && ms == -1,
           "a run that fails in a timed repetition fails the call");
    expect(g_events == 0, "every event is released");
    {
        ugp::EventPair ev(state->stream);
        double acc = 1.0;
        expect(ev.create() == hipSuccess && ev.start() == hipSuccess && ev.lap(&acc) == hipSuccess && ev.lap(&acc) == hipSuccess && acc == 13.0 && g_events == 2,
               "EventPair::lap adds to its accumulator");
    }
    expect(g_events == 0, "EventPair releases its events");
    expect(ugp::query_ready(nullptr, "ugp_stub_run", "stub") == UGP_ERR_INVALID && g_error == "ugp_stub_run: no stub tables: call ugp_stub_attach first" &&
               ugp::query_ready(state, "ugp_stub_run", "stub") == UGP_OK,
           "query_ready names the call, the family and its attach");
    ugp::query_free(state);
    ugp::dfs_tables_free(tables);
    expect(g_states == 0 && g_streams == 0 && g_tables == 0, "query_free destroys the state and its stream");
    return failed;
}
