// The dB / dC folds behind the scan backward (include/caduceus_hip.h): cad_reduce_partials / cad_reduce_partials_multi sum the partial slots
// of a finished launch in one streaming pass; cad_fold_partials_stream folds them chunk by chunk on a second stream WHILE the scan
// backward still runs (placement gate + fold kernel); cad_stream_probe tells whether two streams really run concurrently.
// The scan's geometry -- chunk length, slot depth (cad_scan_bwd_partials), counter layout (cad_scan_bwd_fold_counter_ints) -- is defined
// by scan_bwd.hip and scan_common.h alone; nothing here is compiled into a scan kernel.
#include "scan_common.h"

namespace {

// dst[i] = sum_k src[k * n + i]  (partial slots in T, fp32 accumulation); 4 elements per thread
template <typename T>
__device__ __forceinline__ void ld4p(const T* p, float* o);
template <>
__device__ __forceinline__ void ld4p<float>(const float* p, float* o) {
    struct __attribute__((aligned(16))) V { float f[4]; };
    const V t = *(const V*)p;
    o[0] = t.f[0], o[1] = t.f[1], o[2] = t.f[2], o[3] = t.f[3];
}
template <>
__device__ __forceinline__ void ld4p<bf16_t>(const bf16_t* p, float* o) {
    struct __attribute__((aligned(8))) V { uint32_t w[2]; };
    const V t = *(const V*)p;
    o[0] = cad_bits2f(t.w[0] << 16), o[1] = cad_bits2f(t.w[0] & 0xffff0000u);
    o[2] = cad_bits2f(t.w[1] << 16), o[3] = cad_bits2f(t.w[1] & 0xffff0000u);
}

// T = the destination's element type; the slots are in cad_slot_of<T> (bf16 for an fp16 destination)
template <typename T>
__global__ void reduce_partials_kernel(const typename cad_slot_of<T>::type* src, int nparts, int64_t n, T* dst, int vec) {
    typedef typename cad_slot_of<T>::type TS;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x * 4;
    for (int64_t i = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 4; i < n; i += stride) {
        // (the library's one summation order, include/caduceus_hip.h: groups of CAD_FOLD_GROUP consecutive slots, then the group sums)
        if (vec && i + 4 <= n) {
            float s[4] = {0.f, 0.f, 0.f, 0.f};
            for (int k0 = 0; k0 < nparts; k0 += CAD_FOLD_GROUP) {
                float g[4] = {0.f, 0.f, 0.f, 0.f};
                for (int k = k0; k < nparts && k < k0 + CAD_FOLD_GROUP; ++k) {
                    float x[4];
                    ld4p<TS>(src + (int64_t)k * n + i, x);
                    g[0] += x[0], g[1] += x[1], g[2] += x[2], g[3] += x[3];
                }
                s[0] += g[0], s[1] += g[1], s[2] += g[2], s[3] += g[3];
            }
            cad_cvt_store<T, 4>(dst + i, s);
        } else {
            for (int64_t q = i; q < n && q < i + 4; ++q) {
                float acc = 0.f;
                for (int k0 = 0; k0 < nparts; k0 += CAD_FOLD_GROUP) {
                    float g = 0.f;
                    for (int k = k0; k < nparts && k < k0 + CAD_FOLD_GROUP; ++k) g += to_f32(src[(int64_t)k * n + q]);
                    acc += g;
                }
                dst[q] = from_f32<T>(acc);
            }
        }
    }
}

// Deep and narrow fp32 folds: the add + norm weight gradient of a long sequence is 1024 slots of d_model floats.  reduce_partials_kernel
// gives every thread one 4-float column and ALL slots of it: 64 threads of the whole GPU walk 1 MB in 128 dependent rounds of loads
// (0.27 ms per layer; the fold of a 0.23 ms kernel).  Here a workgroup owns RPD_VPB neighbouring columns (64 contiguous bytes of every
// slot) and its threads the slot GROUPS of them: thread t sums the CAD_FOLD_GROUP slots of group t / RPD_VPB (+ 64, + 128, ...) in slot
// order with all eight loads in flight, the group sums go through LDS, and one thread per column adds them in group order -- the
// library's one summation order, bit-identical to reduce_partials_kernel.
#define RPD_T 256
#define RPD_VPB 4
#define RPD_MAX_GROUPS 512   // 32 KB of LDS: slot depths up to 4096
#define RPD_MIN_PARTS 64
#define RPD_MAX_N 65536      // (a wide fold has a thread per column to fill the GPU with: reduce_partials_kernel)
__global__ __launch_bounds__(RPD_T) void reduce_partials_deep_kernel(const float* src, int nparts, int64_t n, float* dst) {
    struct __attribute__((aligned(16))) V4 { float f[4]; };
    __shared__ V4 gs[RPD_MAX_GROUPS][RPD_VPB];
    const int t = threadIdx.x, v = t % RPD_VPB;
    const int64_t i = ((int64_t)blockIdx.x * RPD_VPB + v) * 4;  // (n % 4 == 0: i < n means the whole column is inside)
    const int ngroups = (nparts + CAD_FOLD_GROUP - 1) / CAD_FOLD_GROUP;
    if (i < n) {
        for (int grp = t / RPD_VPB; grp < ngroups; grp += RPD_T / RPD_VPB) {
            const int k0 = grp * CAD_FOLD_GROUP;
            float x[CAD_FOLD_GROUP][4];
#pragma unroll
            for (int k = 0; k < CAD_FOLD_GROUP; ++k) {
                if (k0 + k < nparts) ld4p<float>(src + (int64_t)(k0 + k) * n + i, x[k]);
                else x[k][0] = x[k][1] = x[k][2] = x[k][3] = 0.f;
            }
            V4 g = {{0.f, 0.f, 0.f, 0.f}};
#pragma unroll
            for (int k = 0; k < CAD_FOLD_GROUP; ++k)
                if (k0 + k < nparts) g.f[0] += x[k][0], g.f[1] += x[k][1], g.f[2] += x[k][2], g.f[3] += x[k][3];
            gs[grp][v] = g;
        }
    }
    __syncthreads();
    if (t < RPD_VPB && i < n) {
        float s[4] = {0.f, 0.f, 0.f, 0.f};
        for (int grp = 0; grp < ngroups; ++grp) {
            const V4 g = gs[grp][v];
            s[0] += g.f[0], s[1] += g.f[1], s[2] += g.f[2], s[3] += g.f[3];
        }
        cad_cvt_store<float, 4>(dst + i, s);
    }
}

// several folds of the same depth and length in one launch (blockIdx.y = job): the dB and dC slots of both parameter sets of a layer
struct ReduceJobs {
    const void* src[CAD_REDUCE_MAX_JOBS];
    void* dst[CAD_REDUCE_MAX_JOBS];
};
template <typename T>
__global__ void reduce_partials_multi_kernel(ReduceJobs jobs, int nparts, int64_t n) {
    typedef typename cad_slot_of<T>::type TS;
    const TS* src = (const TS*)jobs.src[blockIdx.y];
    T* dst = (T*)jobs.dst[blockIdx.y];
    const int64_t stride = (int64_t)gridDim.x * blockDim.x * 4;
    for (int64_t i = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 4; i < n; i += stride) {  // (n % 4 == 0, 16-byte aligned: checked)
        float s[4] = {0.f, 0.f, 0.f, 0.f};
        for (int k0 = 0; k0 < nparts; k0 += CAD_FOLD_GROUP) {
            float g[4] = {0.f, 0.f, 0.f, 0.f};
            for (int k = k0; k < nparts && k < k0 + CAD_FOLD_GROUP; ++k) {
                float x[4];
                ld4p<TS>(src + (int64_t)k * n + i, x);
                g[0] += x[0], g[1] += x[1], g[2] += x[2], g[3] += x[3];
            }
            s[0] += g[0], s[1] += g[1], s[2] += g[2], s[3] += g[3];
        }
        cad_cvt_store<T, 4>(dst + i, s);
    }
}

// ---- the dB / dC fold behind a RUNNING scan backward (cad_fold_partials_stream, include/caduceus_hip.h) -----------------------------
// One workgroup per (slice x of a chunk, row, parameter set), 256 threads.  A 512-position chunk of a row's dB / dC is 2 N rows x 512
// bf16; slice x is elements [x EPW, (x + 1) EPW) of it, EPW = 2 N 512 / n_partials (256 at configs[2]: half a row).  Per slot the
// slice is VPS = EPW / 8 16-byte vectors; thread t owns vector t % VPS of the CAD_FOLD_GROUP = 8 slots of group t / VPS (8 loads in
// flight per thread, 32 KB per workgroup), sums them in slot order, and the first VPS threads add the group sums in group order
// through LDS: the library's one summation order, bit-identical to cad_reduce_partials_multi.  Chunks are taken in the order the scan
// produces them (last logical chunk first); a right-to-left row's logical chunk c lies at physical positions L - (c + 1) 512.
#define FOLD_T 256
#define FOLD_CHUNK 512
static_assert(FOLD_CHUNK == SC_STATE_STEP, "the fold walks the scan backward's chunks (scan_common.h)");
struct FoldSets {
    cad_fold_args s[SC_MAXSETS];
};
// Placement gate.  The fold kernel must reach a CU AFTER the scan workgroup it shares that CU with: a 48-VGPR / 10 KB allocation that
// lands first -- or next to the waves of a third kernel that then leave (the carry pass of an L-split backward, an RCCL all-reduce) --
// sits in the MIDDLE of the register file / LDS and leaves no contiguous 2 x 232 VGPRs / 132 KB for the scan workgroup: measured, the
// full pass of an L-split backward did not start until the fold gave up 20 ms later (profiles/r06_ab_stream_fold.txt).  So one wave runs
// AHEAD of the fold kernel on its stream and returns only when the scan's workgroups have been placed: every scan workgroup adds 1 to
// counters[SB x nchunks] as it starts; the gate waits for the first arrival, then until the count has stopped rising for ~20 us (a whole
// grid is dispatched within a microsecond; a launch with more workgroups than CUs stalls at the resident ones) or the budget is spent.
__global__ __launch_bounds__(64) void fold_gate_kernel(FoldSets sets, int nsets, int want, uint64_t budget_ticks) {
    if (threadIdx.x != 0) return;
    const uint64_t t0 = cad_wall_clock();
    int last = -1;
    uint64_t t_change = t0;
    for (;;) {
        int n = 0;
        for (int i = 0; i < nsets; ++i) {
            const cad_fold_args& a = sets.s[i];
            n += cad_counter_load_agent(a.counters + a.SB * (a.L / FOLD_CHUNK));
        }
        const uint64_t now = cad_wall_clock();
        if (n >= want) return;
        if (n != last) last = n, t_change = now;
        if (n > 0 && now - t_change >= 2000) return;   // 20 us without a new workgroup: everything that fits is resident
        if (now - t0 >= budget_ticks) return;          // the scan is not running next to us: the fold kernel deals with that itself
        cad_poll_sleep();
    }
}

#define FOLD_MAX_ITEMS 256  // items (slice, row, set) one workgroup may be given
#define FOLD_WAKE_DIV 4     // wake this fraction of the predicted period early
__global__ __launch_bounds__(FOLD_T) void fold_stream_kernel(FoldSets sets, int nsets, int mode, uint64_t budget_ticks) {
    // One launch has AT MOST one workgroup per CU (the host passes the CU count as the grid limit): a second resident fold workgroup would
    // take the registers the next scan workgroup needs on that CU (2 x 232 + 2 x 48 > 512 VGPRs per SIMD) and starve the scan of launches
    // with more workgroups than CUs (configs[4]: measured +19 % per layer with one fold workgroup per item).  Items beyond the grid are
    // taken by the same workgroups, item = blockIdx.x + j gridDim.x -- in the order the scan's workgroups are dispatched, and never
    // blocking on one item while another has a chunk ready.
    __shared__ float part[FOLD_T / 2 * 8];
    __shared__ int nextc[FOLD_MAX_ITEMS];  // next chunk of item j (chunks are taken from the last logical one down); < 0: done
    __shared__ int pick_s[2];              // {item to fold now or -1, give up}
    const int t = threadIdx.x;
    const cad_fold_args& a0 = sets.s[0];
    const int G = a0.n_partials, N = a0.N;
    const int64_t L = a0.L, SB = a0.SB;
    const int64_t nchunks = L / FOLD_CHUNK;
    const int total = G * (int)SB * nsets;
    const int nitems = (total - (int)blockIdx.x + (int)gridDim.x - 1) / (int)gridDim.x;
    const int EPW = 2 * N * FOLD_CHUNK / G, VPS = EPW / 8, NG = G / CAD_FOLD_GROUP;  // NG x VPS = 16 N threads work (all 256 at d_state 16)
    const bool active = t < NG * VPS;
    const int v = t % VPS, grp = active ? t / VPS : 0;
    const int64_t part_stride = (int64_t)N * SB * L;
    auto item_set = [&](int j) { return (blockIdx.x + j * gridDim.x) / (G * (int)SB); };
    auto item_row = [&](int j) { return ((blockIdx.x + j * gridDim.x) / G) % (int)SB; };
    auto item_slice = [&](int j) { return (blockIdx.x + j * gridDim.x) % G; };
    auto abort_slot = [&](int j) -> int* {
        const cad_fold_args& a = sets.s[item_set(j)];
        return a.abort_from ? a.abort_from + (int64_t)item_row(j) * G + item_slice(j) : nullptr;
    };
    if (mode == CAD_FOLD_CONCURRENT) {
        // co-location check (see scan_bwd_kernel): not next to a scan workgroup AND scan workgroups still unplaced -> this workgroup is
        // in their way (its registers / LDS sit where theirs must go): hand everything to the cleanup launch and leave
        if (t == 0) {
            int started = 0, here = 0;
            const int key = cad_cu_key();
            for (int i = 0; i < nsets; ++i) {
                const int* base = sets.s[i].counters + sets.s[i].SB * nchunks;
                started += cad_counter_load_agent(base);
                here += cad_counter_load_agent(base + 1 + key);
            }
            pick_s[0] = (here == 0 && started < total) ? 1 : 0;
        }
        __syncthreads();
        if (pick_s[0]) {
            for (int j = t; j < nitems; j += FOLD_T) {
                int* as = abort_slot(j);
                if (as) *as = (int)nchunks;
            }
            return;
        }
        __syncthreads();  // pick_s is rewritten below
    }
    for (int j = t; j < nitems; j += FOLD_T) {
        int c = (int)nchunks - 1;
        if (mode == CAD_FOLD_CLEANUP) {  // what a concurrent pass left (stored as chunk + 1: 0 = nothing)
            int* as = abort_slot(j);
            c = (as ? *as : 0) - 1;
            if (as) *as = 0;
        }
        nextc[j] = c;
    }
    __syncthreads();
    int first = 0;  // (thread 0 only) items before `first` are done
    uint64_t t_last = (mode == CAD_FOLD_CONCURRENT && t == 0) ? cad_wall_clock() : 0;
    // Polling costs the scan next door (every poll is a load through the CU's memory pipeline that its staging waves wait on: same-box
    // A/B, layer 7.60 -> 7.49 ms with 4x longer sleeps): thread 0 learns the cadence of the arrivals (a chunk every ~13 us) and sleeps
    // through most of the predicted gap after a fold -- one or two failed polls per chunk instead of five to ten.
    uint64_t period = 0;       // ticks between the last two picks that had to wait (0: unknown)
    uint64_t t_wake = 0;       // do not poll before this time
    for (;;) {
        // ---- choose: the first item (in dispatch order) whose next chunk is complete; at most 4 pending items are polled per round
        if (t == 0) {
            int pick = -1, give_up = 0, alive = 0;
            while (first < nitems && nextc[first] < 0) ++first;
            bool waited = false;
            for (;;) {
                if (mode == CAD_FOLD_CONCURRENT && t_wake) {
                    while (cad_wall_clock() < t_wake) cad_poll_sleep();
                    t_wake = 0;
                }
                int polled = 0;
                alive = 0;
                for (int j = first; j < nitems && pick < 0 && polled < 4; ++j) {
                    const int c = nextc[j];
                    if (c < 0) continue;
                    alive = 1;
                    if (mode != CAD_FOLD_CONCURRENT) {
                        pick = j;
                    } else {
                        const cad_fold_args& a = sets.s[item_set(j)];
                        ++polled;
                        if (cad_counter_load_agent(a.counters + (int64_t)item_row(j) * nchunks + c) >= G) pick = j;
                    }
                }
                if (pick >= 0 || !alive) break;
                if (cad_wall_clock() - t_last >= budget_ticks) {  // no arrival anywhere for the whole budget: not co-scheduled with a
                    give_up = 1;                                  // progressing scan -- leave the rest to the cleanup launch
                    break;
                }
                waited = true;
                cad_poll_sleep();
            }
            if (pick >= 0 && mode == CAD_FOLD_CONCURRENT) {
                const uint64_t now = cad_wall_clock();
                if (waited) {  // steady state: this chunk arrived while we were watching -- the next one is a period away
                    if (t_last) period = now - t_last;
                    if (period > 5000) period = 5000;           // (50 us: never sleep long on a stale estimate)
                    t_wake = now + period - period / FOLD_WAKE_DIV;  // wake a fraction of the period early
                }
                t_last = now;
            }
            pick_s[0] = pick, pick_s[1] = give_up;
        }
        __syncthreads();
        const int j = cad_uniform(pick_s[0]);  // (workgroup-uniform: everything derived from the item stays in scalar registers)
        if (j < 0) {
            if (pick_s[1]) {
                for (int q = t; q < nitems; q += FOLD_T) {
                    int* as = abort_slot(q);
                    if (nextc[q] >= 0 && as) *as = nextc[q] + 1;
                }
            }
            return;  // everything folded, or given up
        }
        const int64_t c = cad_uniform(nextc[j]);
        // ---- fold chunk c of item j
        const cad_fold_args& a = sets.s[item_set(j)];
        const int x = item_slice(j);
        const int64_t sb = item_row(j);
        const int e0 = x * EPW + v * 8, r = e0 / FOLD_CHUNK, p = e0 % FOLD_CHUNK;
        const int ten = cad_uniform((x * EPW) / (N * FOLD_CHUNK));  // a slice (EPW divides N 512) never straddles the two tensors: per WORKGROUP
        const int n = r % N;
        const int rev = sb < a.split ? a.rev_lo : a.rev_hi;
        const int64_t cphys = rev ? L - (c + 1) * FOLD_CHUNK : c * FOLD_CHUNK;
        // element offsets inside one tensor's slots fit 32 bits (the launcher checks n_partials N SB L 2 < 2^32): lane arithmetic in 32 bits
        const uint32_t row_off = ((uint32_t)n * (uint32_t)SB + (uint32_t)sb) * (uint32_t)L + (uint32_t)p + (uint32_t)cphys;
        // slot k of the lane's group at (workgroup-uniform base of the tensor + k part_stride, scalar registers) + a 32-bit lane offset
        const char* tbase = (const char*)(ten ? a.dC_slots : a.dB_slots);
        const uint32_t voff = ((uint32_t)(grp * CAD_FOLD_GROUP) * (uint32_t)part_stride + row_off) * 2u;
        char* dbase = (char*)(ten ? a.dC : a.dB);
        float s[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        if (active) {
#pragma unroll
            for (int h = 0; h < 2; ++h) {  // two rounds of four loads: 16 data registers instead of 32
                const void* base[4];
                u32x4 w[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) base[k] = tbase + (int64_t)(4 * h + k) * part_stride * 2;
                cad_load16x4_wt(base, voff, w);
#pragma unroll
                for (int k = 0; k < 4; ++k) {
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        s[2 * q] += cad_bits2f(w[k][q] << 16);
                        s[2 * q + 1] += cad_bits2f(w[k][q] & 0xffff0000u);
                    }
                }
                // the sums of this round exist before the next round's loads are issued (otherwise the scheduler hoists those loads
                // and both rounds' 32 data registers are live at once: 52 instead of 40 VGPRs)
#pragma unroll
                for (int q = 0; q < 8; ++q) cad_order_point(s[q]);
            }
        }
        // group sums through LDS in two rounds (groups 1 .. NG/2 - 1, then NG/2 .. NG - 1): half the staging area -- 4 KB next to the
        // resident scan workgroup's 132 KB -- same order of additions
        const int gh = NG / 2;
        if (active && grp > 0 && grp < gh) {
#pragma unroll
            for (int q = 0; q < 8; ++q) part[(grp * VPS + v) * 8 + q] = s[q];
        }
        __syncthreads();
        if (active && grp == 0) {
#pragma unroll
            for (int q = 0; q < 8; ++q) s[q] = 0.f + s[q];  // (group 0 first: the accumulator of the group sums starts from 0)
#pragma unroll 1
            for (int g = 1; g < gh; ++g) {  // (not unrolled: the kernel must fit the 48 VGPRs two resident scan waves leave on a SIMD)
#pragma unroll
                for (int q = 0; q < 8; ++q) s[q] += part[(g * VPS + v) * 8 + q];
            }
        }
        __syncthreads();
        if (active && grp > 0 && grp >= gh) {
#pragma unroll
            for (int q = 0; q < 8; ++q) part[((grp - gh) * VPS + v) * 8 + q] = s[q];
        }
        __syncthreads();
        if (active && grp == 0) {
#pragma unroll 1
            for (int g = (gh > 1 ? gh : 1); g < NG; ++g) {
#pragma unroll
                for (int q = 0; q < 8; ++q) s[q] += part[((g - gh) * VPS + v) * 8 + q];
            }
            u32x4 ov;
            ov[0] = cad_pack_bf16x2(s[0], s[1]), ov[1] = cad_pack_bf16x2(s[2], s[3]);
            ov[2] = cad_pack_bf16x2(s[4], s[5]), ov[3] = cad_pack_bf16x2(s[6], s[7]);
            *(u32x4*)(dbase + row_off * 2u) = ov;
        }
        if (t == 0) nextc[j] = (int)c - 1;
        __syncthreads();  // `part`, nextc and pick_s are rewritten by the next round
    }
}

// ---- are two streams really concurrent?  (cad_stream_probe) ---------------------------------------------------------------------------
__global__ __launch_bounds__(64) void stream_probe_wait_kernel(const int* flag, int* result, uint64_t budget_ticks) {
    if (threadIdx.x != 0) return;
    const uint64_t t0 = cad_wall_clock();
    int seen = 0;
    do {
        seen = cad_counter_load_agent(flag) != 0;
        if (!seen) cad_poll_sleep();
    } while (!seen && cad_wall_clock() - t0 < budget_ticks);
    result[0] = seen;
}
__global__ __launch_bounds__(64) void stream_probe_set_kernel(int* flag) {
    if (threadIdx.x == 0) cad_counter_add_agent(flag, 1);
}
}  // namespace

extern "C" int cad_stream_probe(void* stream_a, void* stream_b, int* flag, int* result, int64_t budget_us) {
    CAD_CHECK_ARG(flag && result && budget_us > 0 && budget_us <= 1000000);
    CAD_LAUNCH(stream_probe_wait_kernel, dim3(1), dim3(64), 0, stream_a, (const int*)flag, result,
               (uint64_t)budget_us * CAD_WALL_CLOCK_TICKS_PER_US);
    CAD_LAUNCH(stream_probe_set_kernel, dim3(1), dim3(64), 0, stream_b, flag);
    return cad_after_launch();
}

extern "C" int cad_fold_stream_supported(int N, int n_partials, int64_t L, int dtype) {
    if (dtype != CAD_BF16 || N < 1 || L < FOLD_CHUNK || L % FOLD_CHUNK != 0) return 0;
    if (n_partials < CAD_FOLD_GROUP || n_partials > 2048 || (n_partials & (n_partials - 1)) != 0) return 0;
    const int elems = 2 * N * FOLD_CHUNK;
    if (elems % n_partials != 0) return 0;
    const int epw = elems / n_partials;
    if (epw < 8 || epw % 8 != 0) return 0;
    if (n_partials % CAD_FOLD_GROUP != 0) return 0;  // whole groups of 8 slots
    const int vps = epw / 8;                         // vectors per slot and workgroup; (n_partials / 8) x vps = 16 N threads work
    if ((n_partials / CAD_FOLD_GROUP) * vps > FOLD_T) return 0;    // d_state <= 16
    if (FOLD_CHUNK % epw != 0 && epw % FOLD_CHUNK != 0) return 0;  // a slice lies inside one row, or covers whole rows
    if ((N * FOLD_CHUNK) % epw != 0) return 0;                     // ... and inside one tensor
    return 1;  // (bf16 slots are always the write-through 16-byte stores of the scan backward's packed flush)
}

extern "C" int cad_fold_partials_stream(const cad_fold_args* sets, int nsets, int mode, void* stream) {
    CAD_CHECK_ARG(sets && nsets >= 1 && nsets <= SC_MAXSETS);
    CAD_CHECK_ARG(mode == CAD_FOLD_CONCURRENT || mode == CAD_FOLD_CLEANUP || mode == CAD_FOLD_ALL);
    FoldSets ks;
    for (int i = 0; i < nsets; ++i) {
        const cad_fold_args* a = &sets[i];
        CAD_CHECK_ARG(a->dB_slots && a->dC_slots && a->dB && a->dC && a->SB > 0 && a->SB <= 65535);
        CAD_CHECK_ARG(a->split >= 0 && a->split <= a->SB);
        if (!cad_fold_stream_supported(a->N, a->n_partials, a->L, a->dtype)) return CAD_ERR_UNSUPPORTED;
        CAD_CHECK_ARG((((uintptr_t)a->dB_slots | (uintptr_t)a->dC_slots | (uintptr_t)a->dB | (uintptr_t)a->dC) % 16) == 0);
        if ((int64_t)a->n_partials * a->N * a->SB * a->L * 2 >= ((int64_t)1 << 32)) return CAD_ERR_UNSUPPORTED;  // 32-bit lane offsets (per tensor)
        CAD_CHECK_ARG(mode != CAD_FOLD_CONCURRENT || (a->counters && a->abort_from));
        CAD_CHECK_ARG(mode != CAD_FOLD_CLEANUP || a->abort_from);
        CAD_CHECK_ARG(a->N == sets[0].N && a->n_partials == sets[0].n_partials && a->L == sets[0].L && a->SB == sets[0].SB);
        ks.s[i] = *a;
    }
    for (int i = nsets; i < SC_MAXSETS; ++i) ks.s[i] = sets[0];
    // a poll that sees no arrival for this long gives the chunk (and the rest of the row slice) to the cleanup launch: the scan produces a
    // chunk every ~13 us, so 20 ms means "the scan is not running next to us" (serialised queues, a profiler, a debugger)
    const uint64_t budget = 2000000ull;  // ticks of the 100 MHz wall clock
    const int64_t items = (int64_t)sets[0].n_partials * sets[0].SB * nsets;
    const int cus = cad_cu_count();  // one workgroup per CU at most (see the kernel)
    if (items > (int64_t)cus * FOLD_MAX_ITEMS) return CAD_ERR_UNSUPPORTED;
    dim3 grid((unsigned)(items < cus ? items : cus)), block(FOLD_T);
    if (mode == CAD_FOLD_CONCURRENT)  // (same stream: the fold kernel is dispatched when the gate has returned)
        CAD_LAUNCH(fold_gate_kernel, dim3(1), dim3(64), 0, stream, ks, nsets, (int)items, budget);
    CAD_LAUNCH(fold_stream_kernel, grid, block, 0, stream, ks, nsets, mode, budget);
    return cad_after_launch();
}

extern "C" int cad_reduce_partials(const void* src, int n_partials, int64_t n, void* dst, int dst_dtype, void* stream) {
    CAD_CHECK_ARG(src && dst && n_partials >= 1 && n > 0);
    const int vec = (n % 4) == 0 && (((uintptr_t)src | (uintptr_t)dst) % 16) == 0;
    if (dst_dtype == CAD_F32 && vec && n <= RPD_MAX_N && n_partials >= RPD_MIN_PARTS &&
        (n_partials + CAD_FOLD_GROUP - 1) / CAD_FOLD_GROUP <= RPD_MAX_GROUPS) {  // deep and narrow: the slot groups in parallel
        dim3 grid((unsigned)((n / 4 + RPD_VPB - 1) / RPD_VPB)), block(RPD_T);
        CAD_LAUNCH(reduce_partials_deep_kernel, grid, block, 0, stream, (const float*)src, n_partials, n, (float*)dst);
        return cad_after_launch();
    }
    int64_t nb = (n / 4 + 255) / 256 + 1;
    if (nb > 16384) nb = 16384;
    dim3 grid((unsigned)nb), block(256);
    if (dst_dtype == CAD_F32)
        CAD_LAUNCH((reduce_partials_kernel<float>), grid, block, 0, stream, (const float*)src, n_partials, n, (float*)dst, vec);
    else if (dst_dtype == CAD_BF16)
        CAD_LAUNCH((reduce_partials_kernel<bf16_t>), grid, block, 0, stream, (const bf16_t*)src, n_partials, n, (bf16_t*)dst, vec);
    else if (dst_dtype == CAD_F16)  // bf16 slots (the scan backward's fp16 mode)
        CAD_LAUNCH((reduce_partials_kernel<f16_t>), grid, block, 0, stream, (const bf16_t*)src, n_partials, n, (f16_t*)dst, vec);
    else
        return CAD_ERR_UNSUPPORTED;
    return cad_after_launch();
}

extern "C" int cad_reduce_partials_multi(const cad_reduce_job* jobs, int njobs, int n_partials, int64_t n, int dst_dtype, void* stream) {
    CAD_CHECK_ARG(jobs && njobs >= 1 && njobs <= CAD_REDUCE_MAX_JOBS && n_partials >= 1 && n > 0);
    ReduceJobs kj;
    bool vec = (n % 4) == 0;
    for (int i = 0; i < CAD_REDUCE_MAX_JOBS; ++i) {
        const cad_reduce_job& j = jobs[i < njobs ? i : 0];
        CAD_CHECK_ARG(j.src && j.dst);
        kj.src[i] = j.src, kj.dst[i] = j.dst;
        vec = vec && (((uintptr_t)j.src | (uintptr_t)j.dst) % 16) == 0;
    }
    if (!vec) {  // ragged / unaligned: one plain fold per job
        for (int i = 0; i < njobs; ++i) {
            const int rc = cad_reduce_partials(jobs[i].src, n_partials, n, jobs[i].dst, dst_dtype, stream);
            if (rc != CAD_OK) return rc;
        }
        return CAD_OK;
    }
    int64_t nb = (n / 4 + 255) / 256 + 1;
    if (nb > 16384) nb = 16384;
    dim3 grid((unsigned)nb, (unsigned)njobs), block(256);
    if (dst_dtype == CAD_F32)
        CAD_LAUNCH((reduce_partials_multi_kernel<float>), grid, block, 0, stream, kj, n_partials, n);
    else if (dst_dtype == CAD_BF16)
        CAD_LAUNCH((reduce_partials_multi_kernel<bf16_t>), grid, block, 0, stream, kj, n_partials, n);
    else if (dst_dtype == CAD_F16)
        CAD_LAUNCH((reduce_partials_multi_kernel<f16_t>), grid, block, 0, stream, kj, n_partials, n);
    else
        return CAD_ERR_UNSUPPORTED;
    return cad_after_launch();
}