// What a slab one-call is made of: the collective plumbing of mgps_project_free_surface_slab,
// mgps_extrapolate_velocity_slab and mgps_solid_forces_slab, stated once.  Host code only, no HIP header: tests/cpp/slab_call_check.cpp
// runs it with the ranks as threads.  Two rules hold the ranks together:
//   * every rank takes part in every collective, whatever its own status -- a rank that has failed skips its device work, not its
//     transport calls;
//   * a rank's own failure travels in the next agreement, where every rank learns of it at the same place and leaves together.
// A transport call that itself fails is the exception: the rank leaves at once with MGPS_ERR_COMM (its peers meet the broken
// transport at their next call).  A world of one asks its transport nothing.
#pragma once
#include <algorithm>
#include <chrono>
#include <cstring>

#include "mgps_internal.h"

namespace mgps {

// "<fn>: <what>" as the library's last error; the refusal of a bad argument
inline int refuse(const char *fn, const std::string &what)
{
    setLastGlobalError(std::string(fn) + ": " + what);
    return MGPS_ERR_INVALID_ARGUMENT;
}

struct SlabCall {
    using Clock = std::chrono::steady_clock;
    static double ms(Clock::time_point a, Clock::time_point b) { return std::chrono::duration<double, std::milli>(b - a).count(); }

    const Clock::time_point t0 = Clock::now();
    const char *fn = "";
    mgps_comm cm{};        // the caller's transport at full size: members behind its struct_size read as NULL
    int P = 1, rank = 0;
    int status = MGPS_OK;  // this rank's own; the first failure stays
    std::string message;   // the last text this call published (the library's last error is the process's, ranks may be threads)
    double exchangeMs = 0;

    // leaves `code` with "<fn>: <what>" published, whatever the status
    int leave(int code, const std::string &what)
    {
        message = std::string(fn) + ": " + what;
        setLastGlobalError(message);
        return code;
    }
    // The transport check, before any collective: every rank refuses alike.  upTo: offsetof(mgps_comm, <first member the entry can
    // do without>), the shortest struct it takes.
    int open(const char *name, const mgps_comm *comm, const int *splits, size_t upTo)
    {
        fn = name;
        if (!comm || !splits || comm->struct_size < int(upTo) || comm->struct_size > int(sizeof(mgps_comm)) || !comm->exchange || !comm->allreduce ||
            comm->size < 1 || comm->rank < 0 || comm->rank >= comm->size)
            return leave(MGPS_ERR_INVALID_ARGUMENT, "comm / splits: a mgps_comm with exchange and allreduce and the cuts are required");
        std::memcpy(&cm, comm, size_t(comm->struct_size));
        cm.struct_size = int(sizeof(mgps_comm));
        P = cm.size;
        rank = cm.rank;
        return MGPS_OK;
    }
    void step(int rc)
    {
        if (status == MGPS_OK) status = rc;
    }
    int fail(int code, const std::string &what)
    {
        if (status == MGPS_OK) status = leave(code, what);
        return status;
    }
    // What the ranks agree on between two steps: one sum all-reduce that carries `sums`, the largest of each entry of `maxes` (every
    // rank fills its own slot of a P-wide row, so a sum is a max) and the ranks' statuses the same way.  Every rank calls it at the
    // same places; it returns this rank's failure, or the first failing rank's, or MGPS_OK on every rank together.
    int agree(const char *where, double *sums = nullptr, int nsums = 0, double *maxes = nullptr, int nmaxes = 0)
    {
        if (P == 1) return status;  // (sums and maxima over one rank are what they were)
        std::vector<double> v(size_t(nsums) + size_t(nmaxes + 1) * size_t(P), 0.0);
        std::copy(sums, sums + nsums, v.begin());
        for (int q = 0; q < nmaxes; ++q) v[size_t(nsums) + size_t(q) * P + rank] = maxes[q];
        double *st = v.data() + size_t(nsums) + size_t(nmaxes) * P;
        st[rank] = double(status);
        if (cm.allreduce(cm.user, v.data(), int(v.size()), 0) != 0) return leave(MGPS_ERR_COMM, std::string("all-reduce failed (") + where + ")");
        std::copy(v.begin(), v.begin() + nsums, sums);
        for (int q = 0; q < nmaxes; ++q) {
            const double *row = v.data() + size_t(nsums) + size_t(q) * P;
            maxes[q] = *std::max_element(row, row + P);
        }
        if (status != MGPS_OK) return status;
        for (int r = 0; r < P; ++r)
            if (int(st[r]) != MGPS_OK)
                return leave(int(st[r]), "rank " + std::to_string(r) + " failed (" + where + ", status " + std::to_string(int(st[r])) + ")");
        return MGPS_OK;
    }
    // One exchange with both neighbours (NULL / 0 bytes towards a side without one), timed into exchangeMs.
    int trade(const void *sendLo, size_t nSendLo, void *recvLo, size_t nRecvLo, const void *sendHi, size_t nSendHi, void *recvHi, size_t nRecvHi,
              void *stream, const std::string &what)
    {
        if (P == 1) return MGPS_OK;
        const auto a = Clock::now();
        const int rc = cm.exchange(cm.user, sendLo, nSendLo, recvLo, nRecvLo, sendHi, nSendHi, recvHi, nRecvHi, stream);
        exchangeMs += ms(a, Clock::now());
        return rc == 0 ? MGPS_OK : leave(MGPS_ERR_COMM, "exchange failed (" + what + ")");
    }
};

}  // namespace mgps
