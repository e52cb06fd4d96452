// csrc/po_engine_deal.h alone (no HIP): the deal loop's rule, for 1 to 16 workers and 0, 1, workers - 1 and 3 x workers
// groups.  tests/test_engine_layer_cpu.py builds this under ASan + UBSan and under TSan and expects "ok".
//
// "After the first failure is recorded no worker takes a new group, and a group already taken runs to its end": the deal
// loop records a failure by calling last_error() inside the critical section that also hands out groups, so the flag set
// there splits time exactly.  A group taken before the flag may still be entered after it, once per worker that held one;
// the worker that recorded the failure held none.  So after the flag a worker enters run() at most once, the recording
// worker never, and that is what is asserted: no sleeps, no timing.
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <thread>
#include <vector>

#include "../poreover_amd/csrc/po_engine_deal.h"

namespace {

struct Stat { double busy_ms = 0; int groups = 0; };

thread_local std::string tl_error;   // as the library's message: the failing thread's own
thread_local int tl_worker = -1;     // the worker whose begin ran on this thread

#define CHECK(cond, ...)                                                       \
    do {                                                                       \
        if (!(cond)) {                                                         \
            std::printf("%s:%d: %s: ", __FILE__, __LINE__, #cond);             \
            std::printf(__VA_ARGS__);                                          \
            std::printf("\n");                                                 \
            std::exit(1);                                                      \
        }                                                                      \
    } while (0)

struct Case {
    int workers = 1, groups = 0;
    int fail[2] = {-1, -1}, code[2] = {0, 0};   // groups that fail, with these codes
    int begin_fail = -1, begin_code = 0;        // the worker whose begin fails
};

std::string group_msg(int g, int w) { return "group " + std::to_string(g) + " failed on worker " + std::to_string(w); }
std::string begin_msg(int w) { return "begin failed on worker " + std::to_string(w); }

void run_case(const Case& c) {
    const int W = c.workers, G = c.groups;
    std::vector<std::atomic<int>> ran((size_t)G), ran_by((size_t)G);
    for (int g = 0; g < G; ++g) { ran[g] = 0; ran_by[g] = -1; }
    std::vector<int> begun((size_t)W, 0), count((size_t)W, 0), after((size_t)W, 0);   // each worker writes its own
    std::vector<Stat> stats((size_t)W);
    std::atomic<bool> recorded{false};
    std::atomic<int> recorder{-1};

    const PoDealResult res = po_engine_deal(
        W, G, stats.data(),
        [&](int w) {
            tl_worker = w;
            begun[w] += 1;
            if (w != c.begin_fail) return 0;
            tl_error = begin_msg(w);
            return c.begin_code;
        },
        [&](int w, int g) {
            if (recorded.load()) after[w] += 1;
            CHECK(w == tl_worker, "worker %d's group on worker %d's thread", w, tl_worker);
            CHECK(g >= 0 && g < G, "group %d of %d", g, G);
            ran[g] += 1;
            ran_by[g] = w;
            count[w] += 1;
            for (int i = 0; i < 4; ++i) std::this_thread::yield();
            for (int k = 0; k < 2; ++k)
                if (g == c.fail[k]) {
                    tl_error = group_msg(g, w);
                    return c.code[k];
                }
            return 0;
        },
        [&] {   // inside the deal's critical section, on the failing worker's thread
            CHECK(!recorded.load(), "a second failure was recorded");
            recorded = true;
            recorder = tl_worker;
            return tl_error;
        });

    // the groups that ran: a prefix of the order, each once
    int m = 0;
    while (m < G && ran[m] == 1) ++m;
    for (int g = m; g < G; ++g) CHECK(ran[g] == 0, "group %d ran %d times after group %d did not run", g, (int)ran[g], m);
    int sum = 0;
    for (int w = 0; w < W; ++w) {
        CHECK(begun[w] == 1, "worker %d began %d times", w, begun[w]);
        CHECK(stats[w].groups == count[w], "worker %d: stat %d, ran %d", w, stats[w].groups, count[w]);
        CHECK(stats[w].busy_ms >= 0, "worker %d: busy_ms %g", w, stats[w].busy_ms);
        CHECK(after[w] <= (w == recorder ? 0 : 1), "worker %d entered %d groups after the failure was recorded", w, after[w]);
        sum += count[w];
    }
    CHECK(sum == m, "%d groups ran, the stats say %d", m, sum);

    const bool fails = c.begin_fail >= 0 || (c.fail[0] >= 0 && c.fail[0] < G) || (c.fail[1] >= 0 && c.fail[1] < G);
    if (!fails) {
        CHECK(m == G, "%d of %d groups ran", m, G);
        CHECK(res.rc == 0 && res.worker == -1 && res.message.empty(), "rc %d worker %d '%s'", res.rc, res.worker, res.message.c_str());
        CHECK(!recorded.load(), "a failure was recorded");
        return;
    }
    CHECK(recorded.load() && res.worker == recorder, "worker %d returned, worker %d recorded", res.worker, (int)recorder);
    if (c.begin_fail >= 0 && res.worker == c.begin_fail) {
        CHECK(res.rc == c.begin_code && res.message == begin_msg(c.begin_fail), "rc %d '%s'", res.rc, res.message.c_str());
    } else {   // one of the failing groups: it ran, on the worker named, and the message is that thread's
        int k = -1;
        for (int j = 0; j < 2; ++j)
            if (c.fail[j] >= 0 && c.fail[j] < m && res.rc == c.code[j]) k = j;
        CHECK(k >= 0, "rc %d is no failing group's that ran (%d of %d ran)", res.rc, m, G);
        CHECK(res.worker == ran_by[c.fail[k]], "worker %d, group %d ran on %d", res.worker, c.fail[k], (int)ran_by[c.fail[k]]);
        CHECK(res.message == group_msg(c.fail[k], res.worker), "'%s'", res.message.c_str());
    }
    if (c.begin_fail >= 0) {
        CHECK(count[c.begin_fail] == 0, "worker %d ran %d groups after its begin failed", c.begin_fail, count[c.begin_fail]);
        if (c.fail[0] < 0) CHECK(res.worker == c.begin_fail, "worker %d returned", res.worker);
        if (W == 1) CHECK(m == 0, "%d groups ran", m);
    }
    if (c.fail[0] >= 0 && c.fail[1] < 0 && c.begin_fail < 0)   // one failing group: it is among those that ran
        CHECK(c.fail[0] < m && res.rc == c.code[0], "group %d, %d ran, rc %d", c.fail[0], m, res.rc);
}

}  // namespace

int main() {
    for (int W = 1; W <= 16; ++W)
        for (const int G : {0, 1, W - 1, 3 * W}) {
            Case ok;
            ok.workers = W;
            ok.groups = G;
            run_case(ok);                                   // all OK; zero groups: no run call
            for (const int f : {0, G / 2, G - 1}) {
                if (f < 0 || f >= G) continue;
                Case one = ok;                              // one group fails
                one.fail[0] = f;
                one.code[0] = -7;
                run_case(one);
                Case two = one;                             // two groups fail with different codes
                two.fail[1] = (f + 1 + G / 3) % G;
                two.code[1] = -2;
                if (two.fail[1] != f) run_case(two);
            }
            for (const int bw : {0, W - 1}) {               // begin fails on one worker
                Case b = ok;
                b.begin_fail = bw;
                b.begin_code = -4;
                run_case(b);
            }
        }
    std::printf("ok\n");
    return 0;
}
