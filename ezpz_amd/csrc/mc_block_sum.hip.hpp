// The block sums of the Monte-Carlo section (mc_moments, mc_effects, mc_sobol and mc_factorial), each
// piece once: the order that defines a sum's bits -- the adjacent-pair tree over a block of 256 leaves, on the host and on the
// device, and the round's partials folded left to right by the workgroup that draws the last ticket -- the callers of a closing
// step, the sums' workspace and the skeleton of an entry on the process's plan.  A host-only user (tools/asan_*.cpp, under its
// header's EZPZ_*_HOST_ONLY) takes the host tree and the one caller alone.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#if defined(EZPZ_MCM_HOST_ONLY) || defined(EZPZ_MCE_HOST_ONLY) || defined(EZPZ_SOBOL_HOST_ONLY) || defined(EZPZ_MCF_HOST_ONLY)
#define EZPZ_MCB_HOST_ONLY
#else
#include "system.hpp"
#endif

namespace ezpz {
namespace mcb {

constexpr uint32_t kBlock = 256;  // leaves per block of the sums: fixed by the interface

// the adjacent-pair tree over a block's leaves, in place: the host forms' side of every device sum
inline double pair_tree_256(double* v) {
    for (uint32_t h = 1; h < kBlock; h *= 2)
        for (uint32_t t = 0; t < kBlock; t += 2 * h) v[t] = v[t] + v[t + h];
    return v[0];
}

// ---- the callers of a closing step: who takes which element, and the barrier between its phases -----------------------------------
struct OneCaller {  // a host entry
    __host__ __device__ inline uint32_t id() const { return 0; }
    __host__ __device__ inline uint32_t count() const { return 1; }
    __host__ __device__ inline void sync() const {}
};

#if defined(__HIPCC__) && !defined(EZPZ_MCB_HOST_ONLY)

struct WorkgroupCallers {  // a closing kernel: the 256 threads of its one workgroup
    __device__ inline uint32_t id() const { return threadIdx.x; }
    __device__ inline uint32_t count() const { return blockDim.x; }
    __device__ inline void sync() const { __syncthreads(); }
};

// ---- the device tree ---------------------------------------------------------------------------------------------------------------
// leaf(s): leaf s as a T with operator+.  The tree over the N leaves from s, N a power of two: the left half's sum + the right half's
template <int N, class Leaf>
__device__ __forceinline__ auto pair_sum(Leaf& leaf, uint32_t s) {
    if constexpr (N == 1) {
        return leaf(s);
    } else {
        const auto left = pair_sum<N / 2>(leaf, s);
        return left + pair_sum<N / 2>(leaf, s + N / 2);
    }
}

// The adjacent-pair tree over the leaves [s0, s0 + 8 n8), n8 = 1, 2, .. 32 a power of two: eight leaves by the explicit tree, the
// eights pushed through a five-deep binary counter, which is that tree (l0 .. l4: the pending sums of 8, 16, 32, 64 and 128 leaves).
template <class T, class Leaf>
__device__ inline T tree_sum(Leaf& leaf, uint32_t s0, uint32_t n8) {
    T l0{}, l1{}, l2{}, l3{}, l4{}, out{};
#pragma unroll 1
    for (uint32_t g = 0; g < n8; ++g) {
        T v = pair_sum<8>(leaf, s0 + 8 * g);
        if (!(g & 1u)) {
            l0 = v;
            continue;
        }
        v = l0 + v;
        if (!(g & 2u)) {
            l1 = v;
            continue;
        }
        v = l1 + v;
        if (!(g & 4u)) {
            l2 = v;
            continue;
        }
        v = l2 + v;
        if (!(g & 8u)) {
            l3 = v;
            continue;
        }
        v = l3 + v;
        if (!(g & 16u)) {
            l4 = v;
            continue;
        }
        out = l4 + v;
    }
    // (a shorter tree's last eight has every low bit set: the whole sum was stored at the level of n8's own bit)
    if (n8 == 1) out = l0;
    if (n8 == 2) out = l1;
    if (n8 == 4) out = l2;
    if (n8 == 8) out = l3;
    if (n8 == 16) out = l4;
    return out;
}

// ---- the ticket step ---------------------------------------------------------------------------------------------------------------
// The workgroup's partials are out before its ticket is drawn; whoever draws the round's last one sees every block's.  True in
// every thread of that workgroup, which folds the round and puts the ticket back to 0.
__device__ inline bool last_block(unsigned int* ticket) {
    __shared__ uint32_t s_last;
    __threadfence();
    __syncthreads();
    if (threadIdx.x == 0) s_last = atomicAdd(ticket, 1u) == gridDim.x - 1 ? 1u : 0u;
    __syncthreads();
    if (!s_last) return false;
    __threadfence();
    return true;
}

// the last workgroup's fold of part [blocks][count] into sums [count], left to right (the first round starts them), threads over sums
__device__ inline void fold_partials(const double* part, uint32_t count, bool first_round, double* sums) {
    const uint32_t blocks = gridDim.x;
    for (uint32_t e = threadIdx.x; e < count; e += 256) {
        double sum = first_round ? 0.0 : sums[e];
        // (the sums depend on each other, the loads do not: unrolled, several blocks' partials are in flight at once)
#pragma unroll 8
        for (uint32_t b = 0; b < blocks; ++b) sum += part[(uint64_t)b * count + e];
        sums[e] = sum;
    }
}

#endif  // __HIPCC__ && !EZPZ_MCB_HOST_ONLY

#ifndef EZPZ_MCB_HOST_ONLY

// ---- the sums' workspace: a round's partials and integer counts per block, and the ticket (0 between launches) ---------------------
// Whoever owns one orders the launches that use it (a LaunchOrder beside it) and waits for them before it grows.
struct Work {
    DevBuf<double> part;
    DevBuf<uint32_t> part_n;
    DevBuf<unsigned int> ticket;
    bool grows(uint64_t part_count, uint64_t n_count) const { return part_count > part.cap || n_count > part_n.cap || !ticket.p; }
    int ensure(uint64_t part_count, uint64_t n_count) {
        int rc;
        if ((rc = part.ensure(part_count)) != EZPZ_OK || (rc = part_n.ensure(n_count)) != EZPZ_OK) return rc;
        if (!ticket.p) {
            if ((rc = ticket.ensure(1)) != EZPZ_OK) return rc;
            HIP_TRY(hipMemset(ticket.p, 0, ticket.cap * sizeof(unsigned int)));
        }
        return EZPZ_OK;
    }
};

// ---- an entry without a system -------------------------------------------------------------------------------------------------------
// Its workspace is the process's, one per device (system.hpp: plan_of_device).  A call holds the plan's mutex from its first
// allocation to its last enqueue; a workspace that has to grow waits for the last call's launches first; body(plan) enqueues on
// `stream` behind them.
template <class W>
struct ProcessPlan {
    std::mutex mu;
    LaunchOrder order;  // the completion of the last call's launches
    W work;
    int device = -1;
    uint32_t cus = 0;  // the device's compute units, once units() has asked
    int units(uint32_t& out) {
        if (!cus) {
            int n = 0;
            HIP_TRY(hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, device));
            cus = (uint32_t)std::max(n, 1);
        }
        out = cus;
        return EZPZ_OK;
    }
};

template <class W, class Body, class... Dims>
int on_process_plan(hipStream_t stream, uint32_t grown_stamp, uint32_t launched_stamp, Body&& body, Dims... dims) {
    ProcessPlan<W>* P = nullptr;
    int device = -1;
    if (int rc = plan_of_device(P, device)) return rc;
    std::lock_guard<std::mutex> lock(P->mu);
    P->device = device;
    int rc;
    if (P->work.grows(dims...)) {
        if ((rc = P->order.before_overwrite()) != EZPZ_OK || (rc = P->work.ensure(dims...)) != EZPZ_OK) return rc;
        call_stamp(grown_stamp);
    }
    if ((rc = P->order.order_behind(stream)) != EZPZ_OK || (rc = body(*P)) != EZPZ_OK) return rc;
    call_stamp(launched_stamp);
    return P->order.record(stream);
}

#endif  // !EZPZ_MCB_HOST_ONLY

}  // namespace mcb
}  // namespace ezpz
