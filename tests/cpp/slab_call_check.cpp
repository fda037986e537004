// The collective scaffold of the slab one-calls (csrc/mgps_slab_call.h) without a GPU: the ranks are threads, the transport is an
// in-process mgps_comm (a barrier-based all-reduce, an exchange through shared pointers).  For P = 1, 2, 4 and every choice of a
// failing rank (none included): sums, maxima and halos of a good run, the verdict every rank gets when one fails, a second agreement on
// the same transport, transports that report failure, a world of one that asks nobody, and what open() refuses.
#include <atomic>
#include <condition_variable>
#include <cstdio>
#include <mutex>
#include <thread>

#include "mgps_slab_call.h"
using namespace mgps;

static std::atomic<int> gFailures{0};
#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) {                                                       \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);    \
            ++gFailures;                                                     \
        }                                                                    \
    } while (0)

struct Barrier {
    std::mutex m;
    std::condition_variable cv;
    int P, waiting = 0, generation = 0;
    explicit Barrier(int p) : P(p) {}
    void wait()
    {
        std::unique_lock<std::mutex> lock(m);
        const int g = generation;
        if (++waiting == P) {
            waiting = 0;
            ++generation;
            cv.notify_all();
        } else {
            cv.wait(lock, [&] { return generation != g; });
        }
    }
};
struct Sent {
    const void *lo = nullptr, *hi = nullptr;
    size_t nLo = 0, nHi = 0;
};
struct World {
    int P;
    Barrier barrier;
    std::vector<double *> values;
    std::vector<Sent> sent;
    explicit World(int p) : P(p), barrier(p), values(size_t(p)), sent(size_t(p)) {}
};
struct Rank {
    World *w;
    int rank;
    bool allreduceFails = false, exchangeFails = false;  // the collective is carried out, then reported as failed
    int allreduces = 0, exchanges = 0;
};

static int worldAllreduce(void *user, double *v, int count, int op)
{
    Rank &r = *static_cast<Rank *>(user);
    World &w = *r.w;
    ++r.allreduces;
    w.values[size_t(r.rank)] = v;
    w.barrier.wait();
    std::vector<double> out(v, v + count);
    for (int q = 0; q < w.P; ++q)
        if (q != r.rank)
            for (int i = 0; i < count; ++i) out[size_t(i)] = op == 0 ? out[size_t(i)] + w.values[size_t(q)][i] : std::max(out[size_t(i)], w.values[size_t(q)][i]);
    w.barrier.wait();
    std::copy(out.begin(), out.end(), v);
    return r.allreduceFails ? 1 : 0;
}
static int worldExchange(void *user, const void *sendLo, size_t nSendLo, void *recvLo, size_t nRecvLo, const void *sendHi, size_t nSendHi, void *recvHi,
                         size_t nRecvHi, void *)
{
    Rank &r = *static_cast<Rank *>(user);
    World &w = *r.w;
    ++r.exchanges;
    w.sent[size_t(r.rank)] = Sent{sendLo, sendHi, nSendLo, nSendHi};
    w.barrier.wait();
    if (nRecvLo) {
        const Sent &below = w.sent[size_t(r.rank - 1)];
        CHECK(r.rank > 0 && below.nHi == nRecvLo && recvLo);
        std::memcpy(recvLo, below.hi, nRecvLo);
    }
    if (nRecvHi) {
        const Sent &above = w.sent[size_t(r.rank + 1)];
        CHECK(r.rank + 1 < w.P && above.nLo == nRecvHi && recvHi);
        std::memcpy(recvHi, above.lo, nRecvHi);
    }
    w.barrier.wait();
    return r.exchangeFails ? 1 : 0;
}
static int neverAllreduce(void *user, double *, int, int) { return ++static_cast<Rank *>(user)->allreduces; }
static int neverExchange(void *user, const void *, size_t, void *, size_t, const void *, size_t, void *, size_t, void *) { return ++static_cast<Rank *>(user)->exchanges; }

static mgps_comm commOf(Rank &r)
{
    mgps_comm cm{};
    cm.struct_size = int(sizeof(mgps_comm));
    cm.rank = r.rank;
    cm.size = r.w->P;
    cm.user = &r;
    cm.exchange = worldExchange;
    cm.allreduce = worldAllreduce;
    return cm;
}

static const char *kFn = "slab_call_check";
static const int kCuts[5] = {0, 16, 32, 48, 64};
enum Fault { kNone, kOwnFailure, kAllreduceFails, kExchangeFails };

// what one rank does in one call: a trade, an agreement with two sums and two maxima, then a second call's agreement
static void rankBody(World &w, int rank, Fault fault, int failing)
{
    const int P = w.P;
    Rank me{&w, rank};
    me.allreduceFails = fault == kAllreduceFails && rank == failing;
    me.exchangeFails = fault == kExchangeFails && rank == failing;
    const mgps_comm cm = commOf(me);
    SlabCall c;
    CHECK(c.open(kFn, &cm, kCuts, offsetof(mgps_comm, gather)) == MGPS_OK && c.P == P && c.rank == rank);
    const bool own = fault == kOwnFailure && rank == failing;
    if (own) {
        CHECK(c.fail(MGPS_ERR_ALLOC, "own trouble") == MGPS_ERR_ALLOC);
        CHECK(c.fail(MGPS_ERR_HIP, "later trouble") == MGPS_ERR_ALLOC);  // the first failure stays
        c.step(MGPS_ERR_HIP);
        CHECK(c.status == MGPS_ERR_ALLOC && c.message == std::string(kFn) + ": own trouble");
    }
    // the trade: the first plane down, the last plane up; a failing rank takes part
    const bool lo = rank > 0, hi = rank + 1 < P;
    const double first = 100.0 * rank + 1, last = 100.0 * rank + 2;
    double haloLo = -1, haloHi = -1;
    const int traded = c.trade(lo ? &first : nullptr, lo ? sizeof(double) : 0, lo ? &haloLo : nullptr, lo ? sizeof(double) : 0, hi ? &last : nullptr,
                               hi ? sizeof(double) : 0, hi ? &haloHi : nullptr, hi ? sizeof(double) : 0, nullptr, "plane 7");
    CHECK(haloLo == (lo ? 100.0 * (rank - 1) + 2 : -1) && haloHi == (hi ? 100.0 * (rank + 1) + 1 : -1));
    CHECK(me.exchanges == (P > 1 ? 1 : 0) && (P == 1 || c.exchangeMs >= 0));
    if (me.exchangeFails && P > 1) {
        CHECK(traded == MGPS_ERR_COMM && c.message == std::string(kFn) + ": exchange failed (plane 7)" && c.message == lastGlobalError());
    } else {
        CHECK(traded == MGPS_OK);
    }
    // the agreement
    double sums[2] = {double(rank + 1), 2.5}, maxes[2] = {double((rank * 3) % 4), -1.0 - rank};
    const int rc = c.agree("first", sums, 2, maxes, 2);
    double wantMax = 0;
    for (int q = 0; q < P; ++q) wantMax = std::max(wantMax, double((q * 3) % 4));
    if (!(me.allreduceFails && P > 1))  // (results of a good all-reduce arrive on every rank, a failing one included)
        CHECK(sums[0] == P * (P + 1) / 2.0 && sums[1] == 2.5 * P && maxes[0] == wantMax && maxes[1] == -1.0);
    CHECK(me.allreduces == (P > 1 ? 1 : 0));
    if (me.allreduceFails && P > 1) {
        CHECK(rc == MGPS_ERR_COMM && c.message == std::string(kFn) + ": all-reduce failed (first)");
    } else if (own) {
        CHECK(rc == MGPS_ERR_ALLOC && c.message == std::string(kFn) + ": own trouble");
    } else if (fault == kOwnFailure) {
        CHECK(rc == MGPS_ERR_ALLOC && c.message == std::string(kFn) + ": rank " + std::to_string(failing) + " failed (first, status " + std::to_string(int(MGPS_ERR_ALLOC)) + ")");
    } else {
        CHECK(rc == MGPS_OK);
    }
    // nobody was left behind: the next call on the same transport agrees
    me.allreduceFails = false;
    SlabCall next;
    CHECK(next.open(kFn, &cm, kCuts, offsetof(mgps_comm, gatherv)) == MGPS_OK);
    double one = 1.0;
    CHECK(next.agree("second", &one, 1) == MGPS_OK && one == double(P));
}

static void runWorld(int P, Fault fault, int failing)
{
    World w(P);
    std::vector<std::thread> threads;
    for (int r = 0; r < P; ++r) threads.emplace_back(rankBody, std::ref(w), r, fault, failing);
    for (auto &t : threads) t.join();
}

static void worldOfOneAsksNobody()
{
    World w(1);
    Rank me{&w, 0};
    mgps_comm cm = commOf(me);
    cm.exchange = neverExchange;
    cm.allreduce = neverAllreduce;
    SlabCall c;
    CHECK(c.open(kFn, &cm, kCuts, offsetof(mgps_comm, gather)) == MGPS_OK);
    double sum = 3.0, most = 4.0, plane = 0;
    CHECK(c.trade(nullptr, 0, nullptr, 0, &plane, sizeof(plane), &plane, sizeof(plane), nullptr, "plane") == MGPS_OK && c.exchangeMs == 0);
    CHECK(c.agree("alone", &sum, 1, &most, 1) == MGPS_OK && sum == 3.0 && most == 4.0);
    c.fail(MGPS_ERR_HIP, "own trouble");
    CHECK(c.agree("alone") == MGPS_ERR_HIP && me.exchanges == 0 && me.allreduces == 0);
}

static void openRefuses()
{
    World w(2);
    Rank me{&w, 1};
    const mgps_comm good = commOf(me);
    const size_t upTo = offsetof(mgps_comm, gather);
    auto refused = [&](const mgps_comm *cm, const int *cuts, size_t need) {
        SlabCall c;
        const int rc = c.open(kFn, cm, cuts, need);
        return rc == MGPS_ERR_INVALID_ARGUMENT && c.message.find("cuts are required") != std::string::npos && c.message.rfind(kFn, 0) == 0 &&
               c.message == lastGlobalError();
    };
    CHECK(refused(nullptr, kCuts, upTo));
    CHECK(refused(&good, nullptr, upTo));
    mgps_comm cm = good;
    cm.struct_size = int(upTo) - 1;
    CHECK(refused(&cm, kCuts, upTo));
    cm.struct_size = int(offsetof(mgps_comm, gatherv)) - 1;  // enough for the two light entries, not for the projection
    CHECK(!refused(&cm, kCuts, upTo) && refused(&cm, kCuts, offsetof(mgps_comm, gatherv)));
    cm.struct_size = int(sizeof(mgps_comm)) + 1;
    CHECK(refused(&cm, kCuts, upTo));
    cm = good;
    cm.exchange = nullptr;
    CHECK(refused(&cm, kCuts, upTo));
    cm = good;
    cm.allreduce = nullptr;
    CHECK(refused(&cm, kCuts, upTo));
    for (int rank : {-1, 2}) {
        cm = good;
        cm.rank = rank;
        CHECK(refused(&cm, kCuts, upTo));
    }
    cm = good;
    cm.size = 0;
    CHECK(refused(&cm, kCuts, upTo));
    // a caller compiled before allreduce_device was appended: whatever lies behind its struct_size reads as NULL
    cm = good;
    cm.gatherv = reinterpret_cast<decltype(cm.gatherv)>(&gFailures);
    cm.allreduce_device = reinterpret_cast<decltype(cm.allreduce_device)>(&gFailures);
    cm.exchange2 = reinterpret_cast<decltype(cm.exchange2)>(&gFailures);
    cm.struct_size = int(offsetof(mgps_comm, allreduce_device));
    SlabCall c;
    CHECK(c.open(kFn, &cm, kCuts, offsetof(mgps_comm, gatherv)) == MGPS_OK);
    CHECK(c.cm.struct_size == int(sizeof(mgps_comm)) && c.cm.gatherv == cm.gatherv && !c.cm.allreduce_device && !c.cm.exchange2 && c.cm.exchange == worldExchange);
}

int main()
{
    for (int P : {1, 2, 4}) {
        runWorld(P, kNone, -1);
        for (int failing = 0; failing < P; ++failing)
            for (Fault fault : {kOwnFailure, kAllreduceFails, kExchangeFails}) runWorld(P, fault, failing);
        std::printf("P = %d ok: %d\n", P, gFailures.load() == 0);
    }
    worldOfOneAsksNobody();
    openRefuses();
    if (gFailures.load()) {
        std::printf("slab call check: %d checks FAILED\n", gFailures.load());
        return 1;
    }
    std::printf("slab call check ok\n");
    return 0;
}
