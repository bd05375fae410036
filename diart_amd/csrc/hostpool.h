// Host-side worker pool of the per-stream CPU stages (clustering, aggregation + binarisation).
// The streams of a step are independent, so both stages are a parallel-for over streams; the pool
// keeps its threads between steps (spawning 2 x 8 std::threads per 1.3 ms step cost more than the
// work they did) and hands out stream indices one at a time (streams differ in cost: the number of
// active speakers decides how much of the assignment problem there is).
#pragma once
#include <functional>
#include <string>

// fn(worker, i) for i in [0, n) on at most `threads` threads (the caller is worker 0 and takes part).
// Returns when every index has been processed.  Calls from different host threads are serialised.
void dz_host_parallel(int n, int threads, const std::function<void(int, int)>& fn);

// The threads a batch entry point runs n items on when its caller asks for `requested`: 1 .. n.  Worker indices
// stay below it, so per-worker scratch is sized by it.
inline int dz_host_threads(int requested, int n) { return requested < 1 ? 1 : (requested > n ? n : requested); }

// The same parallel-for over items that can fail: fn(worker, i) returns 0 or an error code.  On one thread the
// items run in order and stop at the first failure; on the pool the items are independent and every one runs.
// Reports the LOWEST failing index, its code and that item's dz_last_error() text, which is thread local and
// therefore copied on the thread that ran the item, before another item's overwrites it.  code == 0: none failed.
struct dz_host_failure {
    int index = -1, code = 0, failed = 0;   // failed: how many items failed
    std::string message;
};
dz_host_failure dz_host_parallel_rc(int n, int threads, const std::function<int(int, int)>& fn);
