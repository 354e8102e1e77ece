// What bounds the kernels that stream a block system's rows (jit_kernel.hip.hpp: fast_wave): the same bytes moved with the same
// occupancy and nothing else -- rows of n_row * 8 = 16 000 bytes, 65 536 of them, 1024 persistent workgroups of 4 wavefronts, 32 KB
// of LDS per workgroup (4 workgroups per CU, 4 wavefronts per SIMD), the next row asked for while this one is worked on, the row
// after next at a fixed stride or DRAWN from a counter two rows ahead as solve_kernel_fast draws it (with its one barrier per row).
// A wavefront owns a contiguous piece of the row as the generator's wave ranges give it for the 2000 x 2000 system: 4096 bytes for
// the first three, the rest (3712) for the last.
//   strided    eight 8-byte accesses per lane at strides of 32 / 16 bytes: a 128-byte line is shared by three or four instructions
//   full-line  16 bytes per lane at 1024 p + 16 lane, through registers (piece_load / piece_store), lanes past the piece masked
//   lds-dma    the next piece by buffer_load ... lds (16 B per lane, 1 KB per instruction) into the wavefront's other LDS buffer,
//              the "work" reads and writes LDS, the stores read LDS: the shape fast_wave<2> would have without ahead[]
//   bounded    the descriptor's base and num_records are the wavefront's piece: the hardware drops what lies outside, no lane masks
//   nt         the non-temporal policy (aux 2) on the loads, the stores or both
// Every variant's output is compared with the input plus the fixed arithmetic, bit for bit, and a guard band behind the last row
// with its fill, BEFORE its time counts; a variant that fails prints FAILED and no time.
// usage: row_copy_bench [rows [row_bytes]]     (row_bytes a multiple of 8; 16 008 makes the last piece 8 mod 16: the clip check)
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>
typedef int v2 __attribute__((ext_vector_type(2)));
typedef int v4 __attribute__((ext_vector_type(4)));
typedef v4 __attribute__((may_alias)) lds_v4;
typedef __attribute__((address_space(3))) void lds_void;
constexpr int kPieces = 4;                      // 1 KB each: a wavefront's piece is at most 4 KB
constexpr int kLdsPerWave = 2 * kPieces * 1024;  // this row's piece and the next one's
constexpr int kLds = 4 * kLdsPerWave;            // 32 KB per workgroup, used or not: the solve kernel's occupancy
constexpr int kGuard = 4096;                     // bytes behind the last row that nobody may touch
constexpr int kTicketStride = 1024;              // words between two counters, as in the solve kernel (4 KB: another channel)

__device__ __forceinline__ __amdgpu_buffer_rsrc_t desc(const void* base, uint32_t bytes) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), 0, (int)bytes, 0x00020000);
}
__device__ __forceinline__ double work(double x) {  // ~600 dependent-ish flops per wavefront and row, like the solve
    for (int it = 0; it < 20; ++it) x = __builtin_fma(x, 1.0000001, 1e-9);
    return x;
}
enum { STRIDED = 0, FULL = 1, DMA = 2 };

struct Args {
    const char* in;
    char* out;
    int rows;
    uint32_t row_bytes, piece_bytes;
    unsigned int* ticket;  // eight counters, kTicketStride words apart, zero at launch
};

template <int MODE, bool BOUND, int LAUX, int SAUX, bool TICKET>
__global__ void __launch_bounds__(256) copy_rows(const Args a) {
    extern __shared__ __attribute__((aligned(16))) char lds[];
    __shared__ unsigned int drawn_lds[2];
    const int tid = threadIdx.x, lane = tid & 63;
    const uint32_t wave = __builtin_amdgcn_readfirstlane((uint32_t)tid >> 6);
    const uint32_t first = wave * a.piece_bytes;
    const uint32_t bytes = first < a.row_bytes ? (a.row_bytes - first < a.piece_bytes ? a.row_bytes - first : a.piece_bytes) : 0u;
    char* const mine = lds + wave * kLdsPerWave;
    // STRIDED: per lane two "class 0" slots (elements 4 l, 4 l + 2 of a 128-line half) and four "class 1" slots (2 l + 1 style)
    int off[8];
    for (int s = 0; s < 2; ++s) {
        const int line = wave * 128 + s * 64 + lane;
        off[2 * s] = (4 * line) * 8;
        off[2 * s + 1] = (4 * line + 2) * 8;
    }
    for (int s = 0; s < 4; ++s) off[4 + s] = (2 * ((int)wave * 256 + s * 64 + lane) + 1) * 8;

    // a row's descriptor for reading / writing this wavefront's share, and where the share starts in it
    auto row_desc = [&](const char* base, uint64_t row) {
        const char* r = base + row * a.row_bytes;
        if (MODE == STRIDED) return desc(r, a.row_bytes);  // (the pattern covers 2048 doubles: what lies past the row is dropped)
        return BOUND ? desc(r + first, bytes) : desc(r, 0xFFFFFFFFu);
    };
    const uint32_t at0 = (MODE != STRIDED && !BOUND) ? first : 0u;
    auto load_regs = [&](double (&x)[8], const __amdgpu_buffer_rsrc_t r) {
        if (MODE == STRIDED) {
            for (int k = 0; k < 8; ++k) x[k] = __builtin_bit_cast(double, __builtin_amdgcn_raw_buffer_load_b64(r, off[k], 0, LAUX));
        } else {
            for (int p = 0; p < kPieces; ++p) {
                const uint32_t at = 1024u * p + 16u * lane;
                v4 t = v4{0, 0, 0, 0};
                if (BOUND || at + 16u <= bytes) {
                    t = __builtin_amdgcn_raw_buffer_load_b128(r, (int)(at0 + at), 0, LAUX);
                } else if (at + 8u <= bytes) {
                    const v2 h = __builtin_amdgcn_raw_buffer_load_b64(r, (int)(at0 + at), 0, LAUX);
                    t.x = h.x, t.y = h.y;
                }
                x[2 * p] = __builtin_bit_cast(double, v2{t.x, t.y});
                x[2 * p + 1] = __builtin_bit_cast(double, v2{t.z, t.w});
            }
        }
    };
    auto store16 = [&](const v4 q, const __amdgpu_buffer_rsrc_t w, const uint32_t at) {
        if (BOUND || at + 16u <= bytes)
            __builtin_amdgcn_raw_buffer_store_b128(q, w, (int)(at0 + at), 0, SAUX);
        else if (at + 8u <= bytes)
            __builtin_amdgcn_raw_buffer_store_b64(v2{q.x, q.y}, w, (int)(at0 + at), 0, SAUX);
    };
    // the next piece straight into LDS: lane l's 16 bytes of 1 KB p land at buf + 1024 p + 16 l (the instruction's own layout).
    // A piece that is 8 mod 16: LDS-DMA has no 8-byte size -- BOUND leaves the last word to the descriptor (clipped per dword or
    // not: the comparison says), masked lanes take the register route for it.
    auto dma = [&](char* buf, const __amdgpu_buffer_rsrc_t r) {
        for (int p = 0; p < kPieces; ++p) {
            const uint32_t at = 1024u * p + 16u * lane;
            if (BOUND || at + 16u <= bytes) {
                // (the instruction's immediate offset would move BOTH addresses: it stays 0, the LDS base carries 1024 p)
                __builtin_amdgcn_raw_ptr_buffer_load_lds(r, (lds_void*)(buf + 1024 * p), 16, (int)(at0 + at), 0, 0, LAUX);
            } else if (at + 8u <= bytes) {
                const v2 h = __builtin_amdgcn_raw_buffer_load_b64(r, (int)(at0 + at), 0, LAUX);
                *reinterpret_cast<v2*>(buf + at) = h;
            }
        }
    };

    unsigned int drawn = 0;
    unsigned int* const counter = a.ticket + (blockIdx.x & 7u) * kTicketStride;
    auto drawn_row = [&](unsigned int d) { return (uint64_t)gridDim.x + (uint64_t)d * 8u + (blockIdx.x & 7u); };
    if (TICKET && tid == 0) drawn = __hip_atomic_fetch_add(counter, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    double x[8], xn[8];
    uint64_t row = blockIdx.x, row_n = row + gridDim.x;
    if (row < (uint64_t)a.rows) {
        if (MODE == DMA) {
            dma(mine, row_desc(a.in, row));
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        } else {
            load_regs(xn, row_desc(a.in, row));
        }
    }
    if (TICKET) {
        if (tid == 0) drawn_lds[1] = drawn;
        __syncthreads();
        row_n = drawn_row(__builtin_amdgcn_readfirstlane(drawn_lds[1]));
    }
    for (unsigned int kp = 0; row < (uint64_t)a.rows; kp ^= 1u) {
        if (TICKET && tid == 0) drawn = __hip_atomic_fetch_add(counter, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const bool next = row_n < (uint64_t)a.rows;
        const __amdgpu_buffer_rsrc_t w = row_desc(a.out, row);
        if (MODE == DMA) {
            char* const cur = mine + kp * (kPieces * 1024);
            char* const nxt = mine + (kp ^ 1u) * (kPieces * 1024);
            // (the stores that read `nxt` a row ago were issued, so their LDS reads have returned: nothing of it is still wanted)
            if (next) dma(nxt, row_desc(a.in, row_n));
            for (int p = 0; p < kPieces; ++p) {  // the slots: values out of the LDS copy and back into it
                lds_v4* const q = reinterpret_cast<lds_v4*>(cur + 1024 * p + 16 * lane);
                const v4 t = *q;
                const v2 lo = __builtin_bit_cast(v2, work(__builtin_bit_cast(double, v2{t.x, t.y})));
                const v2 hi = __builtin_bit_cast(v2, work(__builtin_bit_cast(double, v2{t.z, t.w})));
                *q = v4{lo.x, lo.y, hi.x, hi.y};
            }
            asm volatile("" ::: "memory");  // (the stores read LDS again, as piece_store does behind the slots' writes)
            for (int p = 0; p < kPieces; ++p) store16(*reinterpret_cast<const lds_v4*>(cur + 1024 * p + 16 * lane), w, 1024u * p + 16u * lane);
            // the next piece has arrived once everything but this row's stores has: they were issued behind it, in order
            if (next) {
                if (BOUND)
                    asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
                else
                    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // (masked stores: how many were issued is not known here)
            }
        } else {
            for (int k = 0; k < 8; ++k) x[k] = xn[k];
            if (next) load_regs(xn, row_desc(a.in, row_n));
            for (int k = 0; k < 8; ++k) x[k] = work(x[k]);
            if (MODE == STRIDED) {
                for (int k = 0; k < 8; ++k) __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(v2, x[k]), w, off[k], 0, SAUX);
            } else {
                for (int p = 0; p < kPieces; ++p) {
                    const v2 lo = __builtin_bit_cast(v2, x[2 * p]), hi = __builtin_bit_cast(v2, x[2 * p + 1]);
                    store16(v4{lo.x, lo.y, hi.x, hi.y}, w, 1024u * p + 16u * lane);
                }
            }
        }
        uint64_t row_nn = row_n + gridDim.x;
        if (TICKET) {
            if (tid == 0) drawn_lds[kp] = drawn;
            __syncthreads();
            row_nn = drawn_row(__builtin_amdgcn_readfirstlane(drawn_lds[kp]));
        }
        row = row_n;
        row_n = row_nn;
    }
}

__global__ void fill_rows(double* in, size_t n) {
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) in[i] = 1.0 + (double)(i % 4093) * 0.125;
}
// out == work(in) bit for bit, and the guard band behind the last row still holds its fill (0xA5 bytes)
__global__ void check_rows(const double* in, const double* out, size_t n, size_t guard_doubles, unsigned long long* bad) {
    unsigned long long mine = 0;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n + guard_doubles; i += (size_t)gridDim.x * blockDim.x) {
        const unsigned long long got = __builtin_bit_cast(unsigned long long, out[i]);
        const unsigned long long want = i < n ? __builtin_bit_cast(unsigned long long, work(in[i])) : 0xA5A5A5A5A5A5A5A5ull;
        mine += got != want;
    }
    if (mine) atomicAdd(bad, mine);
}
#define HIP_OK(call)                                                                       \
    do {                                                                                   \
        const hipError_t e_ = (call);                                                      \
        if (e_ != hipSuccess) {                                                            \
            fprintf(stderr, "%s: %s\n", #call, hipGetErrorString(e_));                     \
            exit(2);                                                                       \
        }                                                                                  \
    } while (0)

struct Variant {
    const char* name;
    void (*kernel)(Args);
    int workgroups;
};

int main(int argc, char** argv) {
    const int rows = argc > 1 ? atoi(argv[1]) : 65536;
    const uint32_t row_bytes = argc > 2 ? (uint32_t)atoi(argv[2]) : 16000u;
    if (rows <= 0 || row_bytes % 8 || row_bytes == 0 || row_bytes > 4u * kPieces * 1024u) {
        fprintf(stderr, "rows > 0, row_bytes a multiple of 8 up to %d\n", 4 * kPieces * 1024);
        return 2;
    }
    const uint32_t piece_bytes = kPieces * 1024u;
    const size_t n = (size_t)rows * (row_bytes / 8), total = n * 8;
    char *in, *out;
    unsigned int* ticket;
    unsigned long long* bad;
    HIP_OK(hipMalloc(&in, total + kGuard));
    HIP_OK(hipMalloc(&out, total + kGuard));
    HIP_OK(hipMalloc(&ticket, 8 * kTicketStride * 4));
    HIP_OK(hipMalloc(&bad, 8));
    hipLaunchKernelGGL(fill_rows, dim3(4096), dim3(256), 0, 0, (double*)in, n);
    HIP_OK(hipDeviceSynchronize());
    hipEvent_t e0, e1;
    HIP_OK(hipEventCreate(&e0));
    HIP_OK(hipEventCreate(&e1));
    const Args a{in, out, rows, row_bytes, piece_bytes, ticket};
    const uint32_t last_piece = row_bytes > 3 * piece_bytes ? row_bytes - 3 * piece_bytes : 0u;
    printf("# %d rows of %u bytes, a wavefront's piece %u bytes, the last one's %u (%s16), 256 threads and %d KB of LDS per workgroup; best and median of 10 launches\n",
           rows, row_bytes, piece_bytes, last_piece, last_piece % 16 ? "8 mod " : "a multiple of ", kLds / 1024);
    printf("# for reference: 6.29 TB/s is the published rate of a plain float4 copy on an MI355X\n");
    const Variant full = {"full-line, registers, lane masks (the kernel today)", copy_rows<FULL, false, 0, 0, false>, 1024};
    const Variant variants[] = {
        {"strided 8 B (the kernels' pattern without CONTIG)", copy_rows<STRIDED, false, 0, 0, false>, 768},
        {"strided 8 B (the kernels' pattern without CONTIG)", copy_rows<STRIDED, false, 0, 0, false>, 1024},
        {"strided 8 B (the kernels' pattern without CONTIG)", copy_rows<STRIDED, false, 0, 0, false>, 2048},
        {"strided 8 B, nt loads + nt stores", copy_rows<STRIDED, false, 2, 2, false>, 1024},
        {full.name, full.kernel, 768},
        full,
        {full.name, full.kernel, 2048},
        {"full-line, registers, lane masks, nt loads", copy_rows<FULL, false, 2, 0, false>, 1024},
        {"full-line, registers, lane masks, nt stores", copy_rows<FULL, false, 0, 2, false>, 1024},
        {"full-line, registers, lane masks, nt loads + nt stores", copy_rows<FULL, false, 2, 2, false>, 1024},
        full,
        {"full-line, registers, lane masks, rows drawn (ticket + barrier)", copy_rows<FULL, false, 0, 0, true>, 1024},
        {"full-line, registers, lane masks, rows drawn, nt loads + nt stores", copy_rows<FULL, false, 2, 2, true>, 1024},
        {"full-line, registers, bounded descriptor", copy_rows<FULL, true, 0, 0, false>, 1024},
        {"full-line, registers, bounded descriptor, nt loads + nt stores", copy_rows<FULL, true, 2, 2, false>, 1024},
        full,
        {"lds-dma, lane masks", copy_rows<DMA, false, 0, 0, false>, 1024},
        {"lds-dma, lane masks, nt loads + nt stores", copy_rows<DMA, false, 2, 2, false>, 1024},
        {"lds-dma, bounded descriptor", copy_rows<DMA, true, 0, 0, false>, 1024},
        {"lds-dma, bounded descriptor, nt loads + nt stores", copy_rows<DMA, true, 2, 2, false>, 1024},
        {"lds-dma, bounded descriptor, rows drawn", copy_rows<DMA, true, 0, 0, true>, 1024},
        {"lds-dma, bounded descriptor, rows drawn, nt loads + nt stores", copy_rows<DMA, true, 2, 2, true>, 1024},
        full,
    };
    std::vector<float> full_runs;
    for (const Variant& v : variants) {
        // correctness first: a fresh output and guard band, one launch, compared on the device
        HIP_OK(hipMemset(out, 0xA5, total + kGuard));
        HIP_OK(hipMemset(ticket, 0, 8 * kTicketStride * 4));
        HIP_OK(hipMemset(bad, 0, 8));
        hipLaunchKernelGGL(v.kernel, dim3(v.workgroups), dim3(256), kLds, 0, a);
        hipLaunchKernelGGL(check_rows, dim3(4096), dim3(256), 0, 0, (const double*)in, (const double*)out, n, (size_t)kGuard / 8, bad);
        unsigned long long wrong = 0;
        HIP_OK(hipMemcpy(&wrong, bad, 8, hipMemcpyDeviceToHost));
        if (wrong) {
            printf("%-68s %4d workgroups: FAILED, %llu of %zu doubles differ (no time taken)\n", v.name, v.workgroups, wrong, n + kGuard / 8);
            continue;
        }
        std::vector<float> ms(12);
        for (int rep = 0; rep < 12; ++rep) {
            HIP_OK(hipMemsetAsync(ticket, 0, 8 * kTicketStride * 4));
            HIP_OK(hipEventRecord(e0));
            hipLaunchKernelGGL(v.kernel, dim3(v.workgroups), dim3(256), kLds, 0, a);
            HIP_OK(hipEventRecord(e1));
            HIP_OK(hipEventSynchronize(e1));
            HIP_OK(hipEventElapsedTime(&ms[rep], e0, e1));
        }
        std::sort(ms.begin() + 2, ms.end());  // (the first two launches warm up)
        const float best = ms[2], median = ms[7];
        if (v.kernel == full.kernel && v.workgroups == full.workgroups) full_runs.push_back(best);
        printf("%-68s %4d workgroups: verified, %.4f ms (median %.4f) = %.1f M rows/s, %.2f TB/s read + written\n", v.name, v.workgroups, best, median,
               rows / best / 1e3, 2.0 * total / best / 1e9);
    }
    if (!full_runs.empty()) {
        const float lo = *std::min_element(full_runs.begin(), full_runs.end()), hi = *std::max_element(full_runs.begin(), full_runs.end());
        printf("# the full-line mode at 1024 workgroups, %zu times across this session: %.4f ... %.4f ms, spread %.2f %% -- a variant counts only beyond that\n",
               full_runs.size(), lo, hi, 100.0 * (hi - lo) / lo);
    }
    printf("# lds-dma two pieces ahead: not run -- a third 4 KB buffer per wavefront is 48 KB per workgroup, and 4 workgroups per CU (the headline's\n"
           "#   4 wavefronts per SIMD) need 192 KB of the CU's 160 KB of LDS: it would cost the occupancy it is meant to feed\n");
    return 0;
}
