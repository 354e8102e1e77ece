// Reference dimensions on the device (include/ezpz_amd.h: ezpz_system_measure and its siblings): the kernels.
// Instantiated in measure.hip only.  Every result is a function of (x_b, S_b, record i) alone, every sum runs in one stated
// order on one lane, there is no atomic and no workgroup waits for another.
//
//   measure_row_kernel     ROW: a workgroup takes `group` consecutive systems at a time, whose rows are one contiguous piece of
//                          x: it is staged into LDS with 16-byte loads of consecutive lanes (the piece's first and last double
//                          alone where the piece is not 16-byte aligned), then the lanes run over (system, measurement) pairs in
//                          the order of m_out and gather from LDS.  The record table is staged too when it fits.
//   measure_direct_kernel  DIRECT: rows that do not fit -- grid-stride over (system, measurement), adjacent lanes on adjacent
//                          measurements of one system, 8-byte gathers from global memory, the table from L2.
//   response_kernel        D[b, i, j]: a fixed (b, j) per run of lanes, which then share the row S[b][j][:], lanes over i; the
//                          gradients come from the workspace [batch][n_meas][8] a measure launch stored.
//   stackup_kernel         worst / rss: one lane per (b, i) over the stored D row, ascending j.
//   vjp_sum_kernel         one lane per (b, v) over the variable's (i, slot) pairs in CSR order (a per-destination sum in place
//                          of atomics), gradients from the workspace.
#pragma once
#include <hip/hip_runtime.h>

#include "constraint_measure.hip.hpp"

namespace ezpz {

constexpr uint32_t kMeasRecWords = 9;  // kind | tag << 16 | n_ids << 24, ids[8] (unused ones 0): the packed record, at an odd stride in LDS

struct MeasureArgs {
    const double* x;        // [batch][n_vars]
    const uint32_t* table;  // [n_meas][kMeasRecWords]
    double* m;              // [batch][n_meas] or null
    uint8_t* flags;         // [batch][n_meas] or null
    double* grad;           // [batch][n_meas][8] or null
    uint64_t batch;
    uint32_t n_vars, n_meas;
    uint32_t group;         // ROW: systems a workgroup stages at a time
    uint32_t table_in_lds;  // ROW: the table is staged behind the rows
    uint32_t grad16;        // grad is 16-byte aligned: its eight doubles leave as four 16-byte stores
};

struct MeasXs {
    const double* x;
    __device__ __forceinline__ double operator[](uint32_t id) const { return x[id]; }
};

__device__ __forceinline__ void measure_one(const MeasureArgs& a, const uint32_t* rec, MeasXs xs, uint64_t out) {
    const uint32_t head = rec[0];
    uint32_t ids[8];
#pragma unroll
    for (int s = 0; s < 8; ++s) ids[s] = rec[1 + s];
    double m, g[8];
    const uint32_t fl = measure::con_measure(head & 0xFFFFu, (head >> 16) & 0xFFu, ids, xs, m, g);
    if (a.m) a.m[out] = m;
    if (a.flags) a.flags[out] = (uint8_t)fl;
    if (a.grad && a.grad16) {
        double2* gp = reinterpret_cast<double2*>(a.grad + out * 8);
#pragma unroll
        for (int s = 0; s < 4; ++s) gp[s] = make_double2(g[2 * s], g[2 * s + 1]);
    } else if (a.grad) {
#pragma unroll
        for (int s = 0; s < 8; ++s) a.grad[out * 8 + s] = g[s];
    }
}

__global__ __launch_bounds__(256) void measure_row_kernel(MeasureArgs a) {
    extern __shared__ double2 meas_lds2[];
    double* lds = reinterpret_cast<double*>(meas_lds2);
    const uint32_t n = a.n_vars, nm = a.n_meas, G = a.group;
    // rows: G * n doubles behind one double of parity padding; the table behind them (8-byte aligned is enough for words)
    const uint32_t row_doubles = (G * n + 2 + 1) & ~1u;
    uint32_t* tab = reinterpret_cast<uint32_t*>(lds + row_doubles);
    if (a.table_in_lds) {
        for (uint32_t k = threadIdx.x; k < nm * kMeasRecWords; k += blockDim.x) tab[k] = a.table[k];
    }
    const uint32_t* table = a.table_in_lds ? tab : a.table;
    const uint64_t n_groups = (a.batch + G - 1) / G;
    for (uint64_t grp = blockIdx.x; grp < n_groups; grp += gridDim.x) {
        const uint64_t b0 = grp * G;
        const uint32_t g_here = (uint32_t)((a.batch - b0) < G ? (a.batch - b0) : G);
        const uint64_t first = b0 * n;                       // the piece: x[first, first + count)
        const uint32_t count = g_here * n;
        const uint32_t par = (uint32_t)(first & 1);          // x is 16-byte aligned (checked by the host side): parity of the index
        double* rows = lds + par;                            // rows[k] = x[first + k]; rows + k is 16-byte aligned where x + first + k is
        __syncthreads();                                     // (the previous group's readers, and the table's writers)
        const uint32_t head = par ? 1u : 0u;                 // a leading odd double
        if (head && threadIdx.x == 0 && count) rows[0] = a.x[first];
        const uint32_t pairs = count > head ? (count - head) / 2 : 0;
        const double2* src2 = reinterpret_cast<const double2*>(a.x + first + head);
        double2* dst2 = reinterpret_cast<double2*>(rows + head);
        for (uint32_t k = threadIdx.x; k < pairs; k += blockDim.x) dst2[k] = src2[k];
        const uint32_t done = head + 2 * pairs;
        if (done < count && threadIdx.x == blockDim.x - 1) rows[done] = a.x[first + done];
        __syncthreads();
        const uint32_t work = g_here * nm;
        for (uint32_t k = threadIdx.x; k < work; k += blockDim.x) {
            const uint32_t g = k / nm, i = k - g * nm;
            measure_one(a, table + (size_t)i * kMeasRecWords, MeasXs{rows + (size_t)g * n}, b0 * nm + k);
        }
    }
}

__global__ __launch_bounds__(256) void measure_direct_kernel(MeasureArgs a) {
    const uint64_t total = a.batch * a.n_meas;
    for (uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; k < total; k += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t b = k / a.n_meas;
        const uint32_t i = (uint32_t)(k - b * a.n_meas);
        measure_one(a, a.table + (size_t)i * kMeasRecWords, MeasXs{a.x + b * a.n_vars}, k);
    }
}

struct ResponseArgs {
    const uint32_t* table;
    const double* grad;  // [batch][n_meas][8]
    const double* S;     // [batch][n_param][n_vars]
    const double* tol;   // [n_param] or null
    double* D;           // [batch][n_meas][n_param]
    double* worst;       // [batch][n_meas] or null
    double* rss;
    uint64_t batch;
    uint32_t n_vars, n_meas, n_param;
};

// D[b, i, j] = sum over slot < n_ids of grad[b, i, slot] * S[b, j, ids_i[slot]], slots ascending, from the first product
__global__ __launch_bounds__(256) void response_kernel(ResponseArgs a) {
    const uint64_t total = a.batch * a.n_param * a.n_meas;
    for (uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; k < total; k += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t bj = k / a.n_meas;  // (b, j): i runs fastest, so a run of lanes gathers from one row of S
        const uint32_t i = (uint32_t)(k - bj * a.n_meas);
        const uint64_t b = bj / a.n_param;
        const uint32_t j = (uint32_t)(bj - b * a.n_param);
        const uint32_t* rec = a.table + (size_t)i * kMeasRecWords;
        const uint32_t n_ids = rec[0] >> 24;
        const double* g = a.grad + (b * a.n_meas + i) * 8;
        const double* s = a.S + bj * a.n_vars;
        double acc = g[0] * s[rec[1]];
        for (uint32_t slot = 1; slot < n_ids; ++slot) acc = acc + g[slot] * s[rec[1 + slot]];
        a.D[(b * a.n_meas + i) * a.n_param + j] = acc;
    }
}

// worst[b, i] = sum_j |D| tol_j, rss[b, i] = sqrt(sum_j (D tol_j)^2): ascending j from +0.0, over the stored D row
__global__ __launch_bounds__(256) void stackup_kernel(ResponseArgs a) {
    const uint64_t total = a.batch * a.n_meas;
    for (uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; k < total; k += (uint64_t)gridDim.x * blockDim.x) {
        const double* d = a.D + k * a.n_param;
        double w = 0.0, q = 0.0;
        for (uint32_t j = 0; j < a.n_param; ++j) {
            const double t = a.tol[j], v = d[j];
            w = w + fabs(v) * t;
            const double vt = v * t;
            q = q + vt * vt;
        }
        a.worst[k] = w;
        a.rss[k] = sqrt(q);
    }
}

struct VjpArgs {
    const double* grad;     // [batch][n_meas][8]
    const double* grad_m;   // [batch][n_meas]
    const uint32_t* csr;    // [n_vars + 1] offsets, then the pairs i * 8 + slot, ascending per variable
    double* grad_x;         // [batch][n_vars]
    uint64_t batch;
    uint32_t n_vars, n_meas;
};

__global__ __launch_bounds__(256) void vjp_sum_kernel(VjpArgs a) {
    const uint64_t total = a.batch * a.n_vars;
    const uint32_t* pairs = a.csr + a.n_vars + 1;
    for (uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; k < total; k += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t b = k / a.n_vars;
        const uint32_t v = (uint32_t)(k - b * a.n_vars);
        const double* g = a.grad + b * a.n_meas * 8;
        const double* gm = a.grad_m + b * a.n_meas;
        double acc = 0.0;
        for (uint32_t e = a.csr[v]; e < a.csr[v + 1]; ++e) {
            const uint32_t p = pairs[e];
            acc = acc + gm[p >> 3] * g[p];
        }
        a.grad_x[k] = acc;
    }
}

}  // namespace ezpz
