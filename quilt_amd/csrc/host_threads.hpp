// host_threads.hpp -- how the library's native calls fan host work over threads.  Plain C++ (no HIP): the host-only sources and
// the sanitizer builds of the tests include it as well.
#pragma once

#include <algorithm>
#include <atomic>
#include <cstddef>
#include <cstdlib>
#include <exception>
#include <mutex>
#include <thread>
#include <vector>

namespace qa {

// Host threads one native call may use for its per-chain host work (input validation, tables, block definition): at most
// `cap`, the machine's hardware threads, or QA_HOST_THREADS when the caller sets it (a launcher that runs several ranks and
// several host threads per rank divides the cores between them: bench.py does).
inline int host_threads(int cap = 16) {
    int c = std::min<int>(cap, (int)std::max(1u, std::thread::hardware_concurrency()));
    if (const char *e = getenv("QA_HOST_THREADS")) {
        const int v = atoi(e);
        if (v >= 1) c = std::min(c, v);
    }
    return std::max(c, 1);
}

// f(i) for every i in [0, n) on min(n_thr, n) threads, the calling thread one of them; the indices are handed out one at a time.
// An exception inside a task (std::bad_alloc: the msPBWT index is 0.8 GB at K = 50 000) must not escape its thread -- that is
// std::terminate, and the host is R or Python: the first one is kept, the other tasks are skipped, and it is rethrown on the
// calling thread, whose callers map it to a status with qa::set_error.  A thread that cannot be started is treated the same way,
// and every thread that was started is joined before anything leaves this function.
template <class F>
void parallel_for(size_t n, int n_thr, F f) {
    if (n_thr <= 1 || n <= 1) {
        for (size_t i = 0; i < n; i++) f(i);
        return;
    }
    std::atomic<size_t> next{0};
    std::atomic<bool> failed{false};
    std::exception_ptr err;
    std::mutex mu;
    auto fail = [&] {   // (called from a catch block)
        std::lock_guard<std::mutex> g(mu);
        if (!err) err = std::current_exception();
        failed.store(true);
    };
    auto work = [&] {
        try {
            for (size_t i; !failed.load() && (i = next.fetch_add(1)) < n;) f(i);
        } catch (...) {
            fail();
        }
    };
    std::vector<std::thread> th;
    try {
        const size_t n_spawn = std::min<size_t>((size_t)n_thr, n) - 1;
        th.reserve(n_spawn);
        for (size_t t = 0; t < n_spawn; t++) th.emplace_back(work);
        work();
    } catch (...) {
        fail();
    }
    for (auto &t : th) t.join();
    if (err) std::rethrow_exception(err);
}

}  // namespace qa
