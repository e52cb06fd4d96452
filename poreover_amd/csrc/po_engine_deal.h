// The deal loop of an engine's run (po_engine.h), free of HIP: groups 0 .. n_groups - 1 go, in order, from one counter
// under one mutex to one host thread per worker, whichever is free.  The first failure recorded wins, with the message and
// the index of the thread that recorded it; from then on no worker takes a new group, and a group already taken runs to its
// end.  tools/engine_deal_check.cpp runs this file alone under sanitizers.  Host only, hidden.
#pragma once
#include <chrono>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#pragma GCC visibility push(hidden)

struct PoDealResult {
    int rc = 0;             // 0 (PO_OK), or the first code recorded
    int worker = -1;        // the worker that recorded it
    std::string message;    // last_error() on that worker's thread
};

// begin(w) -> int, once on worker w's thread before its first group (a worker whose begin fails runs nothing and reports
// that code); run(w, g) -> int; last_error() -> std::string, called on the failing worker's thread.  stats[w].busy_ms and
// stats[w].groups grow by what worker w ran.
template <class Stat, class Begin, class RunGroup, class LastError>
PoDealResult po_engine_deal(int n_workers, int n_groups, Stat* stats, Begin begin, RunGroup run, LastError last_error) {
    std::mutex mu;
    int next = 0;
    PoDealResult res;
    auto worker = [&](int w) {
        int rc = begin(w);
        for (;;) {
            int g = -1;
            {
                std::lock_guard<std::mutex> lk(mu);
                if (rc != 0 && res.rc == 0) {   // the first failure: the others finish what they hold, take no more
                    res.rc = rc;
                    res.worker = w;
                    res.message = last_error();
                }
                if (res.rc == 0 && next < n_groups) g = next++;
            }
            if (g < 0) return;
            const auto t0 = std::chrono::steady_clock::now();
            rc = run(w, g);
            stats[w].busy_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
            stats[w].groups += 1;
        }
    };
    std::vector<std::thread> th;
    for (int w = 0; w < n_workers; ++w) th.emplace_back(worker, w);
    for (auto& t : th) t.join();
    return res;
}

#pragma GCC visibility pop
