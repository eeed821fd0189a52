// aux_streams.hip — auxiliary streams for the forked decodes (host code only; declarations in common.h).
#include "common.h"

namespace ldpc {

namespace {
// Auxiliary streams for the forked decodes (the a == 1 rule's pass, the IRA path's Infinity-Cache chunks): kAux
// streams and their fork / join events per (host thread, device, CALLER stream) — keyed by the caller's stream so
// that decodes on different caller streams never share an auxiliary stream (no false dependence of one caller's join
// on another's fork, and a graph capture open on stream A never absorbs a decode issued on stream B), and per host
// thread so that no two threads interleave one set's fork / join.  At most kAuxSets sets per thread (the least
// recently used one outside any open graph capture is destroyed — hipStreamDestroy lets its pending work finish);
// a thread's sets are destroyed when it exits.
constexpr int kAux = 3;
constexpr int kAuxSets = 16;
struct Aux {
    int dev = -1;
    hipStream_t caller = nullptr;
    uint64_t used = 0;  // LRU stamp
    hipStream_t s[kAux] = {};
    hipEvent_t fork = nullptr, join[kAux] = {};
    void release() {
        for (int i = 0; i < kAux; ++i) {
            if (s[i]) (void)hipStreamDestroy(s[i]);
            if (join[i]) (void)hipEventDestroy(join[i]);
            s[i] = nullptr;
            join[i] = nullptr;
        }
        if (fork) (void)hipEventDestroy(fork);
        fork = nullptr;
        dev = -1;
        caller = nullptr;
    }
    bool create() {
        if (hipEventCreateWithFlags(&fork, hipEventDisableTiming) != hipSuccess) {
            fork = nullptr;
            return false;
        }
        for (int i = 0; i < kAux; ++i) {
            if (hipStreamCreateWithFlags(&s[i], hipStreamNonBlocking) != hipSuccess) {
                s[i] = nullptr;
                return false;
            }
            if (hipEventCreateWithFlags(&join[i], hipEventDisableTiming) != hipSuccess) {
                join[i] = nullptr;
                return false;
            }
        }
        return true;
    }
};
struct AuxPool {
    Aux set[kAuxSets];
    uint64_t clock = 0;
    ~AuxPool() {
        for (Aux& a : set)
            if (a.dev >= 0) a.release();
    }
};
bool capturing(hipStream_t s) {
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    return hipStreamIsCapturing(s, &cs) == hipSuccess && cs == hipStreamCaptureStatusActive;
}
bool any_capturing(const Aux& a) {
    for (int i = 0; i < kAux; ++i)
        if (a.s[i] && capturing(a.s[i])) return true;
    return false;
}
Aux* aux_get(hipStream_t caller) {
    static thread_local AuxPool pool;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return nullptr;
    Aux* lru = nullptr;
    for (Aux& a : pool.set) {
        if (a.dev == dev && a.caller == caller) {
            a.used = ++pool.clock;
            return &a;
        }
    }
    // evict the least recently used set whose streams are not part of an open graph capture (destroying one
    // would invalidate that capture); none free: the caller gets an error, not a broken graph
    for (Aux& a : pool.set)
        if ((!lru || a.used < lru->used) && (a.dev < 0 || !any_capturing(a))) lru = &a;
    if (!lru) return nullptr;
    if (lru->dev >= 0) lru->release();
    if (!lru->create()) {
        lru->release();
        return nullptr;
    }
    lru->dev = dev;
    lru->caller = caller;
    lru->used = ++pool.clock;
    return lru;
}
}  // namespace

int aux_fork(hipStream_t st, hipStream_t* s2, int n) {
    Aux* a = aux_get(st);
    if (!a || n < 1 || n > kAux) return set_error(LDPC_EHIP, "auxiliary streams unavailable");
    // an auxiliary stream still inside a capture the caller is not part of (a capture that ended abnormally) would
    // record this decode into that graph
    if (!capturing(st))
        for (int i = 0; i < n; ++i)
            if (capturing(a->s[i])) return set_error(LDPC_EHIP, "auxiliary stream is inside another stream's graph capture");
    if (hipEventRecord(a->fork, st) != hipSuccess) return set_error(LDPC_EHIP, "auxiliary stream: fork failed");
    for (int i = 0; i < n; ++i) {
        if (hipStreamWaitEvent(a->s[i], a->fork, 0) != hipSuccess)
            return set_error(LDPC_EHIP, "auxiliary stream: fork failed");
        s2[i] = a->s[i];
    }
    return LDPC_OK;
}

int aux_join(hipStream_t st, int n) {
    Aux* a = aux_get(st);
    if (!a || n < 1 || n > kAux) return set_error(LDPC_EHIP, "auxiliary streams unavailable");
    for (int i = 0; i < n; ++i)
        if (hipEventRecord(a->join[i], a->s[i]) != hipSuccess || hipStreamWaitEvent(st, a->join[i], 0) != hipSuccess)
            return set_error(LDPC_EHIP, "auxiliary stream: join failed");
    return LDPC_OK;
}

}  // namespace ldpc
