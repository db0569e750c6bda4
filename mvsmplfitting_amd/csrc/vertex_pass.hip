// LBS vertex pass: verts[b] = skin( v_template + shapedirs.beta_b + posedirs.pose_feature_b ) + transl_b
// for every vertex and every problem of a 32-problem chunk.
//
// Restates lbs() steps 1,3,5 of the reference (code/smplx/lbs.py:179,192-203,207-220) and the
// "+ transl" of SMPL.forward (code/smplx/body_models_scale.py:401-403); the joint regression
// J(beta) and the kinematic chain (lbs.py:183,205) are done per problem by the step kernel.
//
// Two kernels: lbs_vertex_pass_split_kernel (default; the contraction as error-compensated split-fp16 products on
// the fp16 matrix pipe, described at its definition below) and lbs_vertex_pass_kernel (exact fp32 MFMA chain,
// MVFIT_EXACT_FP32=1), each with a dense and a 4-pair skinning blend.
//
// MI355X mapping of the exact-fp32 kernel (details and the measured timeline: DESIGN.md 4.1)
//   * one workgroup = one tile of 32 vertices x one chunk of 32 problems, 8 waves, 154 KB LDS.
//   * waves 0-3 own the blendshape contraction [32 problems x 224] . [224 x 32 verts x 3] on the matrix
//     cores in exact fp32 (v_mfma_f32_32x32x2_f32, bitwise an fmaf chain): wave w = k-slice w (56 of the 224
//     rows) of all three coordinate planes, 3 accumulators, 84 MFMAs.  The basis is pre-tiled in HBM in
//     B-operand order so every wave load is one contiguous 1 KiB global_load_dwordx4 covering 4 k-steps;
//     each basis element is read once per chunk.
//   * every wave stages only the operands it reads itself (wave-private LDS regions): no workgroup barrier
//     before the compute phase; load issue order is pinned (coefficients, basis stream, blend operands) and
//     the first MFMA waits for the first basis group only (counted vmcnt).
//   * while the basis streams, all 8 waves compute the skinning transforms T = W . A on the VALU and keep
//     them in registers; k-slice partials then meet in LDS in a fixed order (deterministic), all waves
//     apply T and store.
#include <cstdlib>
#include <type_traits>
#include <utility>
#include <hip/hip_ext.h>
#include "mvfit_device.h"
#include "launchers.h"
#include "fit_plan.h"

namespace mvfit {

#ifdef MVFIT_TIMING
__device__ long long g_vp[16];
#define VP_T(k, t0) do { if (blockIdx.x == 5 && (threadIdx.x & 255) == 0) g_vp[(k) + (threadIdx.x >> 8) * 8] += clock64() - (t0); } while (0)
#else
#define VP_T(k, t0) do { } while (0)
#endif

typedef float floatx16 __attribute__((ext_vector_type(16)));

constexpr int VP_NT = 512;
constexpr int VP_KSPLIT = 4;
constexpr int VP_GPS = KGROUPS / VP_KSPLIT;      // 7 groups of 4 k-steps per slice

// one workgroup per CU (LDS-limited): 2 waves per SIMD, so let the allocator use 256 VGPRs instead of
// spilling to keep a third wave possible
// SPARSE_W: every vertex has at most 4 non-zero skinning weights (true of the SMPL family): the blend reads
// 4 (weight, joint) pairs per vertex (M.wsp_w / M.wsp_j, ascending joint index) instead of the dense 24-column
// row - the same non-zero products in the same order, i.e. bit-identical transforms for 1/6 of the FMAs.
// Asynchronous fit (mvfit_fit): the operands of a pass are a ring slot the optimiser kernel publishes while the pass
// is already queued.  The waiting is done by pass_gate_kernel - ONE workgroup queued in front of each pass on the pass
// stream (216 waiting workgroups per pass cost the optimiser 5 % of its speed; one costs nothing measurable): lane b
// polls the tag of problem b (relaxed agent-scope loads, s_sleep between polls, bounded by the wall clock - on a
// timeout the pass simply runs on what the slot holds).  The kernel boundary behind it is the acquire.
// Service rounds of a fit with the SDF term (pass_gate_copy_kernel: gate, gate_round): a problem's gate word belongs to the optimiser workgroup, which
// rewrites it in front of every round's tag - also in front of round r + 1 while round r's term kernels may still run, when round
// r did not ask for the term and so waited for no answer.  Once the round's tag is seen the word is copied into gate_round, and
// the round's term kernels read the copy: it is written here and only here, the next gate kernel is behind them in stream
// order, so every workgroup of every kernel of a round sees one value per problem.  (A round that asked for the term has its
// problem waiting for the answer: the word read behind its tag is that round's.  The copy of a round that did not ask may
// already be the next round's 1: its kernels then compute an answer nobody waits for, complete and with all tickets returned.)
// (Two kernels over one body: the fits without the term keep the gate kernel they had - no argument, no branch of the copy.)
template <bool COPY_GATE>
__device__ __forceinline__ void pass_gate_body(const unsigned* __restrict__ tag, const unsigned* __restrict__ done_round,
                                               unsigned* __restrict__ stats, unsigned* __restrict__ pass_done, unsigned round, int b_lo, int B,
                                               const int* gate, int* __restrict__ gate_round) {
    const int b = b_lo + blockIdx.x * blockDim.x + threadIdx.x;      // grid covers [b_lo, B); every wave polls its own 64 problems
    const bool mine = b < B;
    const unsigned want = round + 1u;
    // stream order: the pass of round - 1 has finished when this kernel starts - tell the optimiser (back-pressure: it
    // does not overwrite ring slot (round - 1) % nslots ... before this)
    if (blockIdx.x == 0 && threadIdx.x == 0) __hip_atomic_store(pass_done, round, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    unsigned t = want, d = 0u;
    bool timed_out = false;
    const long long t_start = wall_clock64();
    for (;;) {
        if (mine) {
            t = __hip_atomic_load(tag + b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            d = __hip_atomic_load(done_round + b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        // operands of this round are there (a larger tag: a later round already overwrote the slot) | the problem
        // finished before this round
        const bool ok = !mine || t >= want || d <= round;
        if (__all(ok)) break;
        if (wall_clock64() - t_start > 300000) { timed_out = true; break; }            // 3 ms at 100 MHz
        __builtin_amdgcn_s_sleep(8);                              // (round 6: 8 instead of 32 - measured in round 5: the round span 4.74 -> 4.6 us, closures/s unchanged)
    }
    if constexpr (COPY_GATE) {
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");           // (the word is read behind the tag that was published behind it)
        if (mine) gate_round[b] = __hip_atomic_load(gate + b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    const unsigned long long missed = __ballot(mine && d > round && t > want);
    if ((threadIdx.x & 63) == 0) {
        if (missed) atomicAdd(stats + 2, (unsigned)__popcll(missed));
        if (timed_out) atomicAdd(stats + 3, 1u);
    }
}
__global__ void pass_gate_kernel(const unsigned* __restrict__ tag, const unsigned* __restrict__ done_round,
                                 unsigned* __restrict__ stats, unsigned* __restrict__ pass_done, unsigned round, int b_lo, int B) {
    pass_gate_body<false>(tag, done_round, stats, pass_done, round, b_lo, B, nullptr, nullptr);
}
__global__ void pass_gate_copy_kernel(const unsigned* __restrict__ tag, const unsigned* __restrict__ done_round,
                                      unsigned* __restrict__ stats, unsigned* __restrict__ pass_done, unsigned round, int b_lo, int B,
                                      const int* gate, int* __restrict__ gate_round) {
    pass_gate_body<true>(tag, done_round, stats, pass_done, round, b_lo, B, gate, gate_round);
}

hipError_t launch_pass_gate(const DevPose& P, int b_lo, int B, hipStream_t stream, const int* gate, int* gate_round) {
    const dim3 grid((B - b_lo + 63) / 64);
    if (gate && gate_round)
        hipLaunchKernelGGL(pass_gate_copy_kernel, grid, dim3(64), 0, stream, P.tag, P.done_round, P.stats, P.pass_done, P.round, b_lo, B,
                           gate, gate_round);
    else
        hipLaunchKernelGGL(pass_gate_kernel, grid, dim3(64), 0, stream, P.tag, P.done_round, P.stats, P.pass_done, P.round, b_lo, B);
    return hipGetLastError();
}

// In the pass itself: a chunk whose 32 problems had all finished before this round has nothing to compute.
__device__ __forceinline__ bool pass_chunk_live(const DevPose& P, int b0, int B, float* word, int tid) {
    if (!P.tag) return true;
    int* verdict = reinterpret_cast<int*>(word);
    if (tid < 64) {
        const int b = b0 + tid;
        const bool mine = tid < 32 && b < B;
        const unsigned d = mine ? P.done_round[b] : 0u;
        const unsigned long long live = __ballot(mine && d > P.round);
        if (tid == 0) {
            *verdict = live != 0ull;
            if (blockIdx.x == 0) atomicAdd(P.stats + (live ? 0 : 1), 1u);      // chunk passes run / skipped
        }
    }
    __syncthreads();
    const bool run = *verdict != 0;
    __syncthreads();                                   // the word is reused (next chunk / staging)
    return run;
}

// ---------------------------------------------------------------------------------------------------------
// Pieces shared by the three pass kernels (exact-fp32, split-fp16, split-fp16 chunk loop).  All force-inlined: the
// kernels differ in how the operands arrive and in the contraction, not in the skinning blend or the epilogue.
// A thread's blend item: vertices {2 vp2, 2 vp2 + 1} x problem bb, all three rows of T (24 accumulators).
// ---------------------------------------------------------------------------------------------------------
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef f32x2 f32x2_a4 __attribute__((aligned(4)));      // a pair of floats at any float address
typedef int i32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ void vp_blend_zero(float (&tr)[3][2][4]) {
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int e = 0; e < 4; ++e) tr[k][i][e] = 0.f;
}

// T[k][i][:] += sum_t w_t A_b[j_t][k][:] for ONE of the thread's two vertices: the 4 (weight, joint) pairs of a vertex
// with <= 4 non-zero weights, in ascending joint order - the non-zero products of the dense blend in the same order
__device__ __forceinline__ void vp_blend_pairs(float (&tr)[3][2][4], int i, const float* arow, const float4& spw, const int4& spj) {
    const float wq[4] = {spw.x, spw.y, spw.z, spw.w};
    const int jq[4] = {spj.x, spj.y, spj.z, spj.w};
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float4 a = *reinterpret_cast<const float4*>(arow + jq[t] * 12 + 4 * k);
            tr[k][i][0] = fmaf(wq[t], a.x, tr[k][i][0]);
            tr[k][i][1] = fmaf(wq[t], a.y, tr[k][i][1]);
            tr[k][i][2] = fmaf(wq[t], a.z, tr[k][i][2]);
            tr[k][i][3] = fmaf(wq[t], a.w, tr[k][i][3]);
        }
}

// the same, the four pairs taken two at a time: 6 transform rows in flight instead of 12 (the resident pass holds its
// tiles' basis in registers next to this); the products and their order are the same
__device__ __forceinline__ void vp_blend_pairs_2x2(float (&tr)[3][2][4], int i, const float* arow, const float4& spw, const int4& spj) {
    const float wq[4] = {spw.x, spw.y, spw.z, spw.w};
    const int jq[4] = {spj.x, spj.y, spj.z, spj.w};
#pragma unroll
    for (int h = 0; h < 2; ++h) {
#pragma unroll
        for (int t = 2 * h; t < 2 * h + 2; ++t)
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const float4 a = *reinterpret_cast<const float4*>(arow + jq[t] * 12 + 4 * k);
                tr[k][i][0] = fmaf(wq[t], a.x, tr[k][i][0]);
                tr[k][i][1] = fmaf(wq[t], a.y, tr[k][i][1]);
                tr[k][i][2] = fmaf(wq[t], a.z, tr[k][i][2]);
                tr[k][i][3] = fmaf(wq[t], a.w, tr[k][i][3]);
            }
        __builtin_amdgcn_sched_barrier(0);
    }
}

// T[k][i][:] = sum_j W[v_i][j] A_b[j][k][:]  (lbs.py:209-213), all 24 joints; Wt_w = this wave's copy of the tile's weights
__device__ __forceinline__ void vp_blend_dense(float (&tr)[3][2][4], const float* arow, const float* Wt_w, int vp2) {
#pragma unroll 4
    for (int j = 0; j < NJ; ++j) {
        const float2 w = *reinterpret_cast<const float2*>(Wt_w + j * 32 + 2 * vp2);
        const float wv[2] = {w.x, w.y};
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float4 a = *reinterpret_cast<const float4*>(arow + j * 12 + 4 * k);
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                tr[k][i][0] = fmaf(wv[i], a.x, tr[k][i][0]);
                tr[k][i][1] = fmaf(wv[i], a.y, tr[k][i][1]);
                tr[k][i][2] = fmaf(wv[i], a.z, tr[k][i][2]);
                tr[k][i][3] = fmaf(wv[i], a.w, tr[k][i][3]);
            }
        }
    }
}

// MFMA D layout -> LDS partials [slice][coordinate][32 problems][33]: col (vertex) = lane & 31,
// row (problem) = (r & 3) + 8 (r >> 2) + 4 (lane >> 5)
__device__ __forceinline__ void vp_put_partial(float* part, int slice, int kc, const floatx16& acc, int lane) {
    float* pdst = part + ((slice * 3 + kc) * 32) * 33 + (lane & 31);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int b = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
        pdst[b * 33] = acc[r];
    }
}

// all waves: combine the K slices of the contraction in a fixed order (deterministic), undo the basis scale (SCALED:
// a power of two, exact) and apply T: out = skinned position before "+ transl", vps = v_posed (side outputs only)
template <int NSLICE, bool SCALED, bool SIDE = true>
__device__ __forceinline__ void vp_apply(const float* part, const float (&tr)[3][2][4], float* out_l, float* vps_l,
                                         int bb, int vp2, float inv_scale) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int v = 2 * vp2 + i;
        float vp[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            float sm = part[((0 * 3 + k) * 32 + bb) * 33 + v];
#pragma unroll
            for (int q = 1; q < NSLICE; ++q) sm += part[((q * 3 + k) * 32 + bb) * 33 + v];
            vp[k] = SCALED ? sm * inv_scale : sm;
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            out_l[bb * 96 + v * 3 + k] = fmaf(tr[k][i][0], vp[0], fmaf(tr[k][i][1], vp[1], fmaf(tr[k][i][2], vp[2], tr[k][i][3])));
            if (SIDE) vps_l[bb * 96 + v * 3 + k] = vp[k];
        }
    }
}

// coalesced store of x + transl: 32 rows of 96 floats; nvalid = floats of the tile row that exist (last tile); store_nt:
// non-temporal (asynchronous fit, see the split kernel).  Row b0 + b of the output starts at float 3 nv (b0 + b) and a tile
// at an even float of its row: the pairs are 8-byte aligned for an even vertex count (12 * 6890 % 8 == 0) and, with an odd
// count, in the even rows only - in its odd rows they start at 4 mod 8.  So a pair is stored through f32x2_a4, which promises
// the 4 bytes every row has: one global_store_dwordx2 either way (gfx9 under HSA takes multi-dword global accesses at any
// dword address - the compiler itself fuses two adjacent 4-byte stores into this instruction), the code of an even count
// unchanged.  (A float2 store here told the compiler 8 bytes: undefined for an odd count.)
__device__ __forceinline__ void vp_store_rows(float* __restrict__ verts, const float* out_l, const float* tau, int nv, int vbase,
                                              int nvalid, int b0, int B, int tid, bool store_nt) {
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const int i = tid + r * VP_NT;                     // 32 * 48 = 1536 = 3 * 512
        const int b = i / 48, q = i - b * 48;
        if (b0 + b < B) {
            float* dst = verts + ((size_t)(b0 + b) * nv + vbase) * 3 + 2 * q;
            const int k0 = (2 * q) % 3, k1 = (2 * q + 1) % 3;
            float2 o = *reinterpret_cast<const float2*>(out_l + b * 96 + 2 * q);
            o.x += tau[b * 4 + k0];
            o.y += tau[b * 4 + k1];
            if (2 * q + 1 < nvalid) {
                if (store_nt) __builtin_nontemporal_store(__builtin_bit_cast(f32x2, o), reinterpret_cast<f32x2_a4*>(dst));
                else *reinterpret_cast<f32x2_a4*>(dst) = __builtin_bit_cast(f32x2, o);
            } else if (2 * q < nvalid) dst[0] = o.x;
        }
    }
}

// Round 6, rounds with the SDF term: the min / max keys of the tile's stored vertices per problem and axis (the values the store path
// writes: x + transl), reduced over the 16 lanes that share a problem row - the term's front kernel reduces the box from 216 x 6 keys
// per problem instead of from 6890 vertices in each of its 16 workgroups (sdf_term.hip: sdf_box_from_parts; the same box: min / max
// of keys are associative and carry the vertex index).  nv_t = vertices of the tile that exist.
__device__ __forceinline__ void vp_box_parts(unsigned long long* __restrict__ parts, const float* out_l, const float* tau, int ntiles, int tile,
                                             int nv_t, int b0, int B, int tid) {
    const int b = tid >> 4, l = tid & 15;
    unsigned long long kmin[3] = {~0ull, ~0ull, ~0ull}, kmax[3] = {0ull, 0ull, 0ull};
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int vv = l + 16 * h;
        if (vv < nv_t) {
            const unsigned v = (unsigned)(tile * TILE_V + vv);
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                const float x = out_l[b * 96 + vv * 3 + a] + tau[b * 4 + a];         // (the store path's own addition)
                const unsigned long long o = (unsigned long long)ord_bits(x) << 32;
                const unsigned long long lo = o | v, hi = o | (unsigned)~v;
                kmin[a] = lo < kmin[a] ? lo : kmin[a];
                kmax[a] = hi > kmax[a] ? hi : kmax[a];
            }
        }
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) { kmin[a] = row16_key<true>(kmin[a]); kmax[a] = row16_key<false>(kmax[a]); }
    if (l == 0 && b0 + b < B) {
        unsigned long long* q = parts + ((size_t)(b0 + b) * ntiles + tile) * 6;
#pragma unroll
        for (int a = 0; a < 3; ++a) { q[a] = kmin[a]; q[3 + a] = kmax[a]; }
    }
}

// side outputs for the vertices the objective reads (consumed by the step kernel of the chained mode)
__device__ __forceinline__ void vp_side_outputs(const DevModel& M, const DevPose& P, const float* vps_l, const float* out_l,
                                                int sel_s0, int sel_s1, int b0, int B, int tid) {
    const int nsel = sel_s1 - sel_s0;
    for (int i = tid; i < nsel * 96; i += VP_NT) {
        const int sl = i / 96, rem = i - sl * 96, b = rem / 3, k = rem - 3 * b;
        if (b0 + b >= B) continue;
        const int lv = M.tile_sel_local[sel_s0 + sl], slot = M.tile_sel_slot[sel_s0 + sl];
        P.vposed_sel[(size_t)(b0 + b) * NC_MAX + 3 * slot + k] = vps_l[b * 96 + lv * 3 + k];
        P.xs_sel[(size_t)(b0 + b) * NC_MAX + 3 * slot + k] = out_l[b * 96 + lv * 3 + k];
    }
}

template <bool SPARSE_W>
__global__ __launch_bounds__(VP_NT) __attribute__((amdgpu_waves_per_eu(2, 2))) void lbs_vertex_pass_kernel(DevModel M, DevPose P, int B,
                                                                float* __restrict__ verts) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* coefT_l = smem;                          // [KROWS][32]
    float* A_l = coefT_l + KROWS * 32;              // [32][A_STRIDE]
    float* Wt_l = A_l + 32 * A_STRIDE;              // [4 copies][24][32]
    float* tau_l = Wt_l + 4 * NJ * 32;              // [32][4]
    float* part = tau_l + 32 * 4;                   // [KSPLIT][3][32][33]
    float* out_l = part + VP_KSPLIT * 3 * 32 * 33;  // [32 b][96]  skinned positions before "+ transl"
    float* vps_l = out_l + 32 * 96;                 // [32 b][96]  v_posed (only read for the side outputs)

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int tile = blockIdx.x;
    const int chunk = P.chunk0 + blockIdx.y;
    const int b0 = chunk * 32;
    if (!pass_chunk_live(P, b0, B, smem, tid)) return;
    const bool mfma_role = wave < 4;
#ifdef MVFIT_TIMING
    const long long t_start = clock64();
#else
    const long long t_start = 0;
#endif

    // Issue order of a wave: (contraction waves only) v_template row, coefficient slice, the 21 KiB basis
    // stream; then (every wave) the skinning operands of its own blend items.  Each wave stages only what
    // it reads itself (wave-private LDS regions), so there is no workgroup barrier before the compute phase.
    // While the basis stream is in flight ALL eight waves run the skinning blend T = W . A on the VALU
    // (the contraction waves would otherwise just wait for HBM); then waves 0-3 run the MFMA chain.
    // Blend item of a thread: vertices {2 vp, 2 vp + 1} x problem bb, all three rows of T (24 accumulators).
    // (requested now: the side-output loop at the end would otherwise start with a cold dependent load)
    const int sel_s0 = M.tile_sel_start[tile], sel_s1 = M.tile_sel_start[tile + 1];
    const int vp2 = tid & 15, bb = tid >> 4;              // wave w blends problems [4 w, 4 w + 4)
    float vt_init[3] = {0.f, 0.f, 0.f};
    float4 bv[3][VP_GPS];
    float4 c40, c41, c42, c43, c44, c45, c46;
    constexpr int SL4 = (KROWS / VP_KSPLIT) * 32 / 4;     // 448 float4 per coefficient slice
    float4* cdst = reinterpret_cast<float4*>(coefT_l) + (wave & 3) * SL4;
    if (mfma_role) {
#pragma unroll
        for (int kc = 0; kc < 3; ++kc) vt_init[kc] = (wave == 0) ? M.vt_planes[kc * M.nv_pad + tile * TILE_V + (lane & 31)] : 0.f;
        const float4* csrc = reinterpret_cast<const float4*>(P.coefT + (size_t)chunk * KROWS * 32) + wave * SL4;
        c40 = csrc[lane]; c41 = csrc[lane + 64]; c42 = csrc[lane + 128]; c43 = csrc[lane + 192];
        c44 = csrc[lane + 256]; c45 = csrc[lane + 320]; c46 = csrc[lane + 384];
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int g = 0; g < VP_GPS; ++g)
#pragma unroll
            for (int kc = 0; kc < 3; ++kc)
                bv[kc][g] = (reinterpret_cast<const float4*>(M.bs4) + ((size_t)(tile * 3 + kc) * KGROUPS + wave * VP_GPS) * 64 + lane)[g * 64];
        __builtin_amdgcn_sched_barrier(0);
    }
    // copy (wave & 3) of the tile's weights: waves w and w + 4 write the identical words to the same copy,
    // so each may read right after its own writes without waiting for the other
    float* Wt_w = Wt_l + (wave & 3) * NJ * 32;
    float4 spw[2];
    int4 spj[2];
    {
        // A of this wave's 4 problems: 4 x 72 float4 = 288 -> 5 per lane (last partial); W: 192 float4 -> 3 per lane
        const float4* asrc4 = reinterpret_cast<const float4*>(P.Amat + (size_t)(b0 + 4 * wave) * 288);   // Bpad rows exist
        const float4* wsrc = reinterpret_cast<const float4*>(M.wt_tiles + (size_t)tile * NJ * 32);
        // (named registers, not arrays: with the sched_barriers the allocator otherwise parks them in scratch)
        const float4 a40 = asrc4[lane], a41 = asrc4[lane + 64], a42 = asrc4[lane + 128], a43 = asrc4[lane + 192],
                     a44 = asrc4[min(lane + 256, 287)];
        float4 w40, w41, w42;
        float4 sw0, sw1;                                  // sparse: weights of vertices 2 vp2, 2 vp2 + 1
        int4 sj0, sj1;                                    //         and their joint indices
        if (SPARSE_W) {
            sw0 = M.wsp_w[(size_t)tile * TILE_V + 2 * vp2]; sw1 = M.wsp_w[(size_t)tile * TILE_V + 2 * vp2 + 1];
            sj0 = M.wsp_j[(size_t)tile * TILE_V + 2 * vp2]; sj1 = M.wsp_j[(size_t)tile * TILE_V + 2 * vp2 + 1];
        } else {
            w40 = wsrc[lane]; w41 = wsrc[lane + 64]; w42 = wsrc[lane + 128];
        }
        if (wave == 7 && lane < 32) reinterpret_cast<float4*>(tau_l)[lane] = reinterpret_cast<const float4*>(P.tau + (size_t)b0 * 4)[lane];
        __builtin_amdgcn_sched_barrier(0);
        if (mfma_role) {      // counted waits: the coefficient slice has landed while 21 + 8 younger loads are in flight
            cdst[lane] = c40; cdst[lane + 64] = c41; cdst[lane + 128] = c42; cdst[lane + 192] = c43;
            cdst[lane + 256] = c44; cdst[lane + 320] = c45; cdst[lane + 384] = c46;
        }
        auto put_a = [&](int i, const float4& v) {
            if (i < 288) { const int b = i / 72, q = i - b * 72; *reinterpret_cast<float4*>(A_l + (4 * wave + b) * A_STRIDE + 4 * q) = v; }
        };
        put_a(lane, a40); put_a(lane + 64, a41); put_a(lane + 128, a42); put_a(lane + 192, a43); put_a(lane + 256, a44);
        if (!SPARSE_W) {
            reinterpret_cast<float4*>(Wt_w)[lane] = w40;
            reinterpret_cast<float4*>(Wt_w)[lane + 64] = w41;
            reinterpret_cast<float4*>(Wt_w)[lane + 128] = w42;
        }
        spw[0] = sw0; spw[1] = sw1; spj[0] = sj0; spj[1] = sj1;
    }
    wave_lds_fence();
    VP_T(1, t_start);
    // ---- skinning blend T[k][i][:] = sum_j W[v_i][j] A_b[j][k][:]  (lbs.py:209-213), all waves ----
    float tr[3][2][4];
    vp_blend_zero(tr);
    if (SPARSE_W) {
        vp_blend_pairs(tr, 0, A_l + bb * A_STRIDE, spw[0], spj[0]);
        vp_blend_pairs(tr, 1, A_l + bb * A_STRIDE, spw[1], spj[1]);
    } else {
        vp_blend_dense(tr, A_l + bb * A_STRIDE, Wt_w, vp2);
    }
    VP_T(2, t_start);
    // (A workgroup barrier here - blend everywhere first, then MFMA - was measured slower: the fp32 MFMA
    // chain and the VALU blend compete for the same FMA units either way, and overlap hides the skew.)
    if (mfma_role) {
        // ---- blendshape contraction: k-slice `wave` of the three coordinate planes ----
        floatx16 acc[3];
#pragma unroll
        for (int kc = 0; kc < 3; ++kc)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[kc][r] = vt_init[kc];
        const float* asrc = coefT_l + (lane >> 5) * 32 + (lane & 31);
#pragma unroll
        for (int g = 0; g < VP_GPS; ++g) {
            const int kk0 = (wave * VP_GPS + g) * 4;
            const float a0 = asrc[(2 * (kk0 + 0)) * 32];
            const float a1 = asrc[(2 * (kk0 + 1)) * 32];
            const float a2 = asrc[(2 * (kk0 + 2)) * 32];
            const float a3 = asrc[(2 * (kk0 + 3)) * 32];
#pragma unroll
            for (int kc = 0; kc < 3; ++kc) {
                acc[kc] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, bv[kc][g].x, acc[kc], 0, 0, 0);
                acc[kc] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, bv[kc][g].y, acc[kc], 0, 0, 0);
                acc[kc] = __builtin_amdgcn_mfma_f32_32x32x2f32(a2, bv[kc][g].z, acc[kc], 0, 0, 0);
                acc[kc] = __builtin_amdgcn_mfma_f32_32x32x2f32(a3, bv[kc][g].w, acc[kc], 0, 0, 0);
            }
        }
#pragma unroll
        for (int kc = 0; kc < 3; ++kc) vp_put_partial(part, wave, kc, acc[kc], lane);
    }
    VP_T(3, t_start);
    __syncthreads();

    // ---- all waves: combine the k-slices (fixed order) and apply T ----
    vp_apply<VP_KSPLIT, false>(part, tr, out_l, vps_l, bb, vp2, 1.0f);
    VP_T(4, t_start);
    __syncthreads();
    VP_T(5, t_start);

    // ---- store x + transl, then the side outputs for the step kernel ----
    vp_store_rows(verts, out_l, tau_l, M.nv, tile * TILE_V, min(TILE_V, M.nv - tile * TILE_V) * 3, b0, B, tid, false);
    vp_side_outputs(M, P, vps_l, out_l, sel_s0, sel_s1, b0, B, tid);
    VP_T(6, t_start);
#ifdef MVFIT_TIMING
    if (blockIdx.x == 5 && threadIdx.x == 0) g_vp[7] += 1;
#endif
}


// ---------------------------------------------------------------------------------------------------------
// Same pass with the blendshape contraction on the fp16 matrix pipe in error-compensated form.
//
// fp32 MFMA issues at the fp32 vector rate; v_mfma_f32_32x32x16_f16 is 16x faster per multiply-add.  Every
// fp32 operand is split into two fp16 terms, x = hi + lo (hi = fp16(x), lo = fp16(x - hi): 22 significant bits),
// and the product is taken as lo.hi + hi.lo + hi.hi with fp32 accumulation inside the MFMA - each partial
// product (11 x 11 bits) is exact in fp32, the dropped lo.lo term is 2^-22 relative.  The basis is pre-split on
// the host (same 4 bytes per element: hi and lo packed as two fp16), scaled by a power of two (M.bs_scale) so that
// the lo terms of all but negligible elements stay in fp16's normal range; the coefficients are split by the
// step kernel when it publishes them (P.coefH).  3 MFMAs of 32 cycles replace 8 of 64 per 16 k-steps.
//
// Mapping: six contraction waves, wave = coordinate plane c (w % 3) x K-half h (w / 3): 7 blocks of 16 rows,
// one accumulator; A and B operands arrive as ready-made 16-byte lane words (no LDS staging, no conversion).
// All eight waves run the skinning blend as in the exact-fp32 kernel; partials meet in LDS in a fixed order.
// ---------------------------------------------------------------------------------------------------------
typedef _Float16 half8 __attribute__((ext_vector_type(8)));
#ifndef VP_NT_LOADS
#define VP_NT_LOADS 1
#endif
__device__ __forceinline__ float4 nt_load16(const float4* p) {
    return __builtin_bit_cast(float4, __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(p)));
}
constexpr int VP_NBLK = KROWS / 16;             // 14 blocks of 16 k-steps
constexpr int VP_BPW = VP_NBLK / 2;             // 7 per contraction wave

template <bool SPARSE_W>
__global__ __launch_bounds__(VP_NT) __attribute__((amdgpu_waves_per_eu(2, 2))) void lbs_vertex_pass_split_kernel(DevModel M, DevPose P, int B,
                                                                float* __restrict__ verts) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* A_l = smem;                              // [32][A_STRIDE]
    float* Wt_l = A_l + 32 * A_STRIDE;              // [4 copies][24][32]
    float* tau_l = Wt_l + 4 * NJ * 32;              // [32][4]
    float* part = tau_l + 32 * 4;                   // [2 K-halves][3][32][33]
    float* out_l = part + 2 * 3 * 32 * 33;          // [32 b][96]  skinned positions before "+ transl"
    float* vps_l = out_l + 32 * 96;                 // [32 b][96]  v_posed (only read for the side outputs)

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int tile = blockIdx.x;
    const int chunk = P.chunk0 + blockIdx.y;
    const int b0 = chunk * 32;
    if (!pass_chunk_live(P, b0, B, smem, tid)) return;
    const bool stream_nt = VP_NT_LOADS && P.tag != nullptr && !(P.pad_ & 1u);       // uniform
    const bool store_nt = VP_NT_LOADS && P.tag != nullptr && !(P.pad_ & 2u);
    const bool mfma_role = wave < 6;
    const int kc_w = wave % 3, kh_w = wave / 3;
#ifdef MVFIT_TIMING
    const long long t_start = clock64();
#else
    const long long t_start = 0;
#endif
    // (requested now: the side-output loop at the end would otherwise start with a cold dependent load)
    const int sel_s0 = M.tile_sel_start[tile], sel_s1 = M.tile_sel_start[tile + 1];
    const int vp2 = tid & 15, bb = tid >> 4;              // wave w blends problems [4 w, 4 w + 4)
    float vt_init = 0.f;
    float4 ah[VP_BPW], al[VP_BPW], bh[VP_BPW], bl[VP_BPW];
    if (mfma_role) {
        vt_init = (kh_w == 0) ? M.vt_planes[kc_w * M.nv_pad + tile * TILE_V + (lane & 31)] * M.bs_scale : 0.f;
        const float4* ca = P.coefH + ((size_t)(chunk * VP_NBLK + kh_w * VP_BPW) * 2) * 64 + lane;
        const float4* cb = M.bs_h2 + ((size_t)((tile * 3 + kc_w) * VP_NBLK + kh_w * VP_BPW) * 2) * 64 + lane;
#pragma unroll
        for (int g = 0; g < VP_BPW; ++g) { ah[g] = ca[(2 * g) * 64]; al[g] = ca[(2 * g + 1) * 64]; }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        // asynchronous fit: the optimiser kernel runs on the other CUs of this XCD and lives on its L2-resident working
        // set (objective basis rows, Gram matrices, VPoser weights); the basis stream (each element used once per
        // launch) and the vertex stores are then issued non-temporal so that they do not push it out
        for (int g = 0; g < VP_BPW; ++g) {
            bh[g] = stream_nt ? nt_load16(&cb[(2 * g) * 64]) : cb[(2 * g) * 64];
            if (!M.half_basis) bl[g] = stream_nt ? nt_load16(&cb[(2 * g + 1) * 64]) : cb[(2 * g + 1) * 64];
            else bl[g] = make_float4(0.f, 0.f, 0.f, 0.f);
        }
        __builtin_amdgcn_sched_barrier(0);
    }
    float* Wt_w = Wt_l + (wave & 3) * NJ * 32;
    float4 spw[2];
    int4 spj[2];
    {
        const float4* asrc4 = reinterpret_cast<const float4*>(P.Amat + (size_t)(b0 + 4 * wave) * 288);   // Bpad rows exist
        const float4* wsrc = reinterpret_cast<const float4*>(M.wt_tiles + (size_t)tile * NJ * 32);
        const float4 a40 = asrc4[lane], a41 = asrc4[lane + 64], a42 = asrc4[lane + 128], a43 = asrc4[lane + 192],
                     a44 = asrc4[min(lane + 256, 287)];
        float4 w40, w41, w42;
        float4 sw0, sw1;
        int4 sj0, sj1;
        if (SPARSE_W) {
            sw0 = M.wsp_w[(size_t)tile * TILE_V + 2 * vp2]; sw1 = M.wsp_w[(size_t)tile * TILE_V + 2 * vp2 + 1];
            sj0 = M.wsp_j[(size_t)tile * TILE_V + 2 * vp2]; sj1 = M.wsp_j[(size_t)tile * TILE_V + 2 * vp2 + 1];
        } else {
            w40 = wsrc[lane]; w41 = wsrc[lane + 64]; w42 = wsrc[lane + 128];
        }
        if (wave == 7 && lane < 32) reinterpret_cast<float4*>(tau_l)[lane] = reinterpret_cast<const float4*>(P.tau + (size_t)b0 * 4)[lane];
        __builtin_amdgcn_sched_barrier(0);
        auto put_a = [&](int i, const float4& v) {
            if (i < 288) { const int b = i / 72, q = i - b * 72; *reinterpret_cast<float4*>(A_l + (4 * wave + b) * A_STRIDE + 4 * q) = v; }
        };
        put_a(lane, a40); put_a(lane + 64, a41); put_a(lane + 128, a42); put_a(lane + 192, a43); put_a(lane + 256, a44);
        if (!SPARSE_W) {
            reinterpret_cast<float4*>(Wt_w)[lane] = w40;
            reinterpret_cast<float4*>(Wt_w)[lane + 64] = w41;
            reinterpret_cast<float4*>(Wt_w)[lane + 128] = w42;
        }
        spw[0] = sw0; spw[1] = sw1; spj[0] = sj0; spj[1] = sj1;
    }
    wave_lds_fence();
    VP_T(1, t_start);
    // ---- skinning blend (lbs.py:209-213), all waves ----
    float tr[3][2][4];
    vp_blend_zero(tr);
    if (SPARSE_W) {
        vp_blend_pairs(tr, 0, A_l + bb * A_STRIDE, spw[0], spj[0]);
        vp_blend_pairs(tr, 1, A_l + bb * A_STRIDE, spw[1], spj[1]);
    } else {
        vp_blend_dense(tr, A_l + bb * A_STRIDE, Wt_w, vp2);
    }
    VP_T(2, t_start);
    if (mfma_role) {
        // ---- blendshape contraction: plane kc_w, K-half kh_w; small products first ----
        floatx16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = vt_init;
#pragma unroll
        for (int g = 0; g < VP_BPW; ++g) {
            const half8 Ah = __builtin_bit_cast(half8, ah[g]), Al = __builtin_bit_cast(half8, al[g]);
            const half8 Bh = __builtin_bit_cast(half8, bh[g]), Bl = __builtin_bit_cast(half8, bl[g]);
            acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(Al, Bh, acc, 0, 0, 0);
            if (!M.half_basis) acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(Ah, Bl, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(Ah, Bh, acc, 0, 0, 0);
        }
        vp_put_partial(part, kh_w, kc_w, acc, lane);
    }
    VP_T(3, t_start);
    __syncthreads();

    // ---- all waves: combine the two K-halves (fixed order), undo the basis scale, apply T ----
    vp_apply<2, true>(part, tr, out_l, vps_l, bb, vp2, 1.0f / M.bs_scale);        // power of two: exact
    VP_T(4, t_start);
    __syncthreads();
    VP_T(5, t_start);

    // ---- store x + transl, then (chained mode only) the side outputs for the step kernel ----
    vp_store_rows(verts, out_l, tau_l, M.nv, tile * TILE_V, min(TILE_V, M.nv - tile * TILE_V) * 3, b0, B, tid, store_nt);
    if (P.box_part) vp_box_parts(P.box_part, out_l, tau_l, M.ntiles, tile, min(TILE_V, M.nv - tile * TILE_V), b0, B, tid);      // (uniform)
    if (!P.tag) vp_side_outputs(M, P, vps_l, out_l, sel_s0, sel_s1, b0, B, tid);
    VP_T(6, t_start);
#ifdef MVFIT_TIMING
    if (blockIdx.x == 5 && threadIdx.x == 0) g_vp[7] += 1;
#endif
}

// ---------------------------------------------------------------------------------------------------------
// More than 32 problems: one workgroup per vertex tile walks ALL 32-problem chunks with the tile's basis held in
// registers - each basis element is read ONCE per launch whatever the number of problems (the single-chunk kernel
// above, launched per (tile, chunk), re-reads it per chunk).  Per-chunk operands (coefficients, transforms) arrive as
// direct global -> LDS loads requested one chunk ahead; no registers are held while they fly.
// ---------------------------------------------------------------------------------------------------------
template <bool SPARSE_W>
__global__ __launch_bounds__(VP_NT) __attribute__((amdgpu_waves_per_eu(2, 2))) void lbs_vertex_pass_split_loop_kernel(DevModel M, DevPose P, int B,
                                                                float* __restrict__ verts) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* A_l = smem;                              // [32][A_STRIDE]
    float* Wt_l = A_l + 32 * A_STRIDE;              // [4 copies][24][32]
    float* tau_l = Wt_l + 4 * NJ * 32;              // [2 parities][32][4]
    float* part = tau_l + 2 * 32 * 4;               // [2 K-halves][3][32][33]
    float* out_l = part + 2 * 3 * 32 * 33;          // [32 b][96]  skinned positions before "+ transl"
    float* vps_l = out_l + 32 * 96;                 // [32 b][96]  v_posed (only read for the side outputs)
    float4* coef_l = reinterpret_cast<float4*>(vps_l + 32 * 96);   // [VP_NBLK][hi, lo][64 lanes] A operands of the chunk
    float* live_w = reinterpret_cast<float*>(coef_l + VP_NBLK * 2 * 64);   // [4] verdict word of pass_chunk_live

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int tile = blockIdx.x;
    const int nchunks = (B + 31) >> 5;
    const bool stream_nt = VP_NT_LOADS && P.tag != nullptr && !(P.pad_ & 1u);       // uniform
    const bool store_nt = VP_NT_LOADS && P.tag != nullptr && !(P.pad_ & 2u);
    const bool mfma_role = wave < 6;
    const int kc_w = wave % 3, kh_w = wave / 3;
#ifdef MVFIT_TIMING
    const long long t_start = clock64();
#else
    const long long t_start = 0;
#endif
    // (requested now: the side-output loop at the end would otherwise start with a cold dependent load)
    const int sel_s0 = M.tile_sel_start[tile], sel_s1 = M.tile_sel_start[tile + 1];
    const int vp2 = tid & 15, bb = tid >> 4;              // wave w blends problems [4 w, 4 w + 4)

    // ---- per-chunk operands: requested one chunk ahead as direct global -> LDS loads (no registers are held while
    //      they fly: the basis already takes 112 of them) ----
    auto load_operands = [&](int chunk, float* tau_dst) {     // every wave requests its share
        const float4* csrc = P.coefH + (size_t)chunk * VP_NBLK * 2 * 64 + lane;                 // 28 x 1 KiB
        for (int i = wave; i < VP_NBLK * 2; i += VP_NT / 64)
            __builtin_amdgcn_global_load_lds(csrc + i * 64, coef_l + i * 64, 16, 0, 0);
        // the chunk's 32 x 288 transforms are one contiguous 36 KiB block in HBM and (A_STRIDE == 288) in LDS: 36 x 1 KiB
        static_assert(A_STRIDE == 288, "linear copy");
        const float4* asrc = reinterpret_cast<const float4*>(P.Amat + (size_t)chunk * 32 * 288) + lane;      // Bpad rows exist
        for (int i = wave; i < 32 * 288 / 256; i += VP_NT / 64)
            __builtin_amdgcn_global_load_lds(asrc + i * 64, reinterpret_cast<float4*>(A_l) + i * 64, 16, 0, 0);
        if (wave == 7 && lane < 32)
            __builtin_amdgcn_global_load_lds(reinterpret_cast<const float4*>(P.tau + (size_t)chunk * 32 * 4) + lane,
                                             reinterpret_cast<float4*>(tau_dst), 16, 0, 0);
    };

    int chunk = P.chunk0 + (int)blockIdx.y;
    load_operands(chunk, tau_l);
    __builtin_amdgcn_sched_barrier(0);
    // ---- chunk-invariant operands: the basis (B operands, kept in registers over all chunks of this workgroup:
    //      each basis element is read ONCE per launch whatever the number of problems), v_template, skinning weights ----
    float vt_init = 0.f;
    float4 bh[VP_BPW], bl[VP_BPW];
    if (mfma_role) {
        vt_init = (kh_w == 0) ? M.vt_planes[kc_w * M.nv_pad + tile * TILE_V + (lane & 31)] * M.bs_scale : 0.f;
        const float4* cb = M.bs_h2 + ((size_t)((tile * 3 + kc_w) * VP_NBLK + kh_w * VP_BPW) * 2) * 64 + lane;
        // asynchronous fit: the optimiser kernel runs on the other CUs of this XCD and lives on its L2-resident working
        // set (objective basis rows, Gram matrices, VPoser weights); the basis stream (each element used once per
        // launch) and the vertex stores are then issued non-temporal so that they do not push it out
#pragma unroll
        for (int g = 0; g < VP_BPW; ++g) {
            bh[g] = stream_nt ? nt_load16(&cb[(2 * g) * 64]) : cb[(2 * g) * 64];
            if (!M.half_basis) bl[g] = stream_nt ? nt_load16(&cb[(2 * g + 1) * 64]) : cb[(2 * g + 1) * 64];
            else bl[g] = make_float4(0.f, 0.f, 0.f, 0.f);
        }
        __builtin_amdgcn_sched_barrier(0);
    }
    float* Wt_w = Wt_l + (wave & 3) * NJ * 32;
    // 4-pair skinning table of the tile's 32 vertices: kept in LDS (the Wt_l area is free in this variant), read at
    // the blend - 16 registers less to hold across the chunk loop next to the 112 of the basis
    float4* sw_l = reinterpret_cast<float4*>(Wt_l);
    int4* sj_l = reinterpret_cast<int4*>(Wt_l + 32 * 4);
    {
        const float4* wsrc = reinterpret_cast<const float4*>(M.wt_tiles + (size_t)tile * NJ * 32);
        if (SPARSE_W) {
            if (tid < 32) sw_l[tid] = M.wsp_w[(size_t)tile * TILE_V + tid];
            else if (tid < 64) sj_l[tid - 32] = M.wsp_j[(size_t)tile * TILE_V + tid - 32];
        } else {
            const float4 w40 = wsrc[lane], w41 = wsrc[lane + 64], w42 = wsrc[lane + 128];
            reinterpret_cast<float4*>(Wt_w)[lane] = w40;
            reinterpret_cast<float4*>(Wt_w)[lane + 64] = w41;
            reinterpret_cast<float4*>(Wt_w)[lane + 128] = w42;
        }
        __builtin_amdgcn_sched_barrier(0);
    }
    const float inv_scale = 1.0f / M.bs_scale;        // power of two: exact
    const int vbase = tile * TILE_V;
    const int nvalid = min(TILE_V, M.nv - vbase) * 3;      // floats valid in this tile row

    for (int it = 0; chunk < nchunks; ++it) {
        const int b0 = chunk * 32;
        const int next = chunk + (int)gridDim.y;
#ifdef MVFIT_TIMING
        const long long t_it = clock64();               // timeline of the second chunk (steady state), tests/vp_timeline.py
#define VPL_T(k_) do { if (it == 1) VP_T(k_, t_it); } while (0)
#else
#define VPL_T(k_) do { } while (0)
#endif
        float* tau_c = tau_l + (it & 1) * 32 * 4;
        float* tau_n = tau_l + ((it + 1) & 1) * 32 * 4;
        if (!pass_chunk_live(P, b0, B, live_w, tid)) {            // uniform; all its problems finished earlier
            if (next < nchunks) load_operands(next, tau_n);
            chunk = next;
            continue;
        }
        // ---- this chunk's operands have been requested one chunk ago: wait for this wave's share, then the barrier
        //      makes every wave's share (the coefficients are staged by all of them) visible ----
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        VPL_T(0);
        __syncthreads();
        VPL_T(1);
        // ---- skinning blend (lbs.py:209-213), all waves ----
        float tr[3][2][4];
        vp_blend_zero(tr);
        if (SPARSE_W) {
            vp_blend_pairs(tr, 0, A_l + bb * A_STRIDE, sw_l[2 * vp2], sj_l[2 * vp2]);
            __builtin_amdgcn_sched_barrier(0);            // 12 transform rows in flight at a time, not 24 (registers)
            vp_blend_pairs(tr, 1, A_l + bb * A_STRIDE, sw_l[2 * vp2 + 1], sj_l[2 * vp2 + 1]);
        } else {
            vp_blend_dense(tr, A_l + bb * A_STRIDE, Wt_w, vp2);
        }
        VPL_T(2);
        __builtin_amdgcn_sched_barrier(0);                    // the blend's LDS reads stay above, the A operands below
        if (mfma_role) {
            // ---- blendshape contraction: plane kc_w, K-half kh_w; small products first.  The A operands come from
            //      LDS two blocks ahead of their MFMAs (not all 14 words at once: the basis holds 112 registers) ----
            floatx16 acc;
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[r] = vt_init;
            const float4* cl = coef_l + (kh_w * VP_BPW * 2) * 64 + lane;
            float4 ah[VP_BPW], al[VP_BPW];
#pragma unroll
            for (int g = 0; g < VP_BPW; ++g) { ah[g] = cl[(2 * g) * 64]; al[g] = cl[(2 * g + 1) * 64]; }
#pragma unroll
            for (int g = 0; g < VP_BPW; ++g) {
                const half8 Ah = __builtin_bit_cast(half8, ah[g]), Al = __builtin_bit_cast(half8, al[g]);
                const half8 Bh = __builtin_bit_cast(half8, bh[g]), Bl = __builtin_bit_cast(half8, bl[g]);
                acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(Al, Bh, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(Ah, Bl, acc, 0, 0, 0);      // (Bl = 0 with MVFIT_HALF_BASIS: the registers here are too tight for a second code path)
                acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(Ah, Bh, acc, 0, 0, 0);
            }
            vp_put_partial(part, kh_w, kc_w, acc, lane);
        }
        VPL_T(3);
        __syncthreads();
        // every MFMA wave has consumed this chunk's coefficients, this wave has blended its transforms: request the
        // next chunk's operands now - they fly under the epilogue and the stores of this one
        if (next < nchunks) load_operands(next, tau_n);

        // ---- all waves: combine the two K-halves (fixed order), undo the basis scale, apply T ----
        vp_apply<2, true>(part, tr, out_l, vps_l, bb, vp2, inv_scale);
        VPL_T(4);
        __syncthreads();
        VPL_T(5);

        // ---- store x + transl, then (chained mode only) the side outputs for the step kernel ----
        vp_store_rows(verts, out_l, tau_c, M.nv, vbase, nvalid, b0, B, tid, store_nt);
        if (!P.tag) vp_side_outputs(M, P, vps_l, out_l, sel_s0, sel_s1, b0, B, tid);
        VPL_T(6);
        // No barrier at the loop end: the next iteration starts with one (behind this wave's operand wait).
        chunk = next;
    }
#ifdef MVFIT_TIMING
    if (blockIdx.x == 5 && threadIdx.x == 0) g_vp[7] += 1;
#endif
}

// ---------------------------------------------------------------------------------------------------------
// More than 32 problems, models with <= 4 skinning weights per vertex (the SMPL family): the chunk loop as a two-role
// software pipeline.  The loop kernel above does blend -> contraction -> apply -> store in lock-step with three barriers
// per chunk and has every wave stall on the issue of the next chunk's 64 KiB of operands (the CU takes ~40 B/clk): 4.2 us
// per 32-problem chunk, of which the matrix pipe works 0.6.  Here
//   * waves 0-2 own one coordinate plane each: its basis rows stay in registers for the whole launch (112 VGPRs), per
//     chunk 42 MFMAs (two K halves, two accumulators added in the order of the other kernels: bit-identical vertices),
//     the partial to LDS - and they are the LOADERS: right behind the second barrier of chunk c they request the operands
//     of chunk c + 2 (direct global -> LDS, 22 x 1 KiB per wave) into the buffer chunk c just released.  Operands are
//     double-buffered (2 x 64 KiB), so a request has a whole iteration to land and is waited for with a COUNTED vmcnt
//     (everything but the newest 22): nobody stalls on the stream;
//   * waves 3-7 (320 threads) own the 512 (vertex pair, problem) items of a chunk: skinning blend T = W . A from the
//     4-pair table (registers), then - behind the barrier that publishes the partials - v_posed, skinned position,
//     "+ transl" and the store straight from registers (24 contiguous bytes per item, 384-byte runs per problem): no
//     staging of the output in LDS, no third barrier.  Blend of chunk c runs WHILE the planes of chunk c are contracted.
// Two barriers per chunk; per chunk the critical path is max(loader: request + 42 MFMAs, worker: 2 blends + 2 applies).
// LDS: A 2 x 36 KiB, coefficients 2 x 28 KiB, partials 12.4 KiB, tau / tables 2 KiB = 143 KiB.
// ---------------------------------------------------------------------------------------------------------
constexpr int VPP_NMFMA = 3;                         // loader / contraction waves
constexpr int VPP_NWORK = (VP_NT / 64 - VPP_NMFMA) * 64;   // 320 worker threads
constexpr int VPP_DMA_PER_WAVE = 22;                 // (28 coefficient + 36 transform + 1 tau + 1 pad) KiB-loads / 3 waves

// LDS accesses of the loader waves go through inline asm: the compiler's wait-count pass cannot tell which LDS bytes an
// in-flight global -> LDS load will write and would put `s_waitcnt vmcnt(0)` in front of every ds instruction that
// follows one - i.e. it would wait for the request of the chunk AFTER next at the top of every iteration.  The waits are
// placed by hand instead (lds_wait* ties the loaded registers to the counter wait so that no use can be scheduled above it).
typedef float f32x4v __attribute__((ext_vector_type(4)));
__device__ __forceinline__ f32x4v lds_read16_nowait(unsigned addr) {
    f32x4v v;
    asm volatile("ds_read_b128 %0, %1" : "=v"(v) : "v"(addr));
    return v;
}
__device__ __forceinline__ void lds_write4_nowait(unsigned addr, float v) {
    asm volatile("ds_write_b32 %0, %1" :: "v"(addr), "v"(v) : "memory");
}
__device__ __forceinline__ void lds_wait14(f32x4v (&a)[14]) {
    asm volatile("s_waitcnt lgkmcnt(0)"
                 : "+v"(a[0]), "+v"(a[1]), "+v"(a[2]), "+v"(a[3]), "+v"(a[4]), "+v"(a[5]), "+v"(a[6]), "+v"(a[7]), "+v"(a[8]),
                   "+v"(a[9]), "+v"(a[10]), "+v"(a[11]), "+v"(a[12]), "+v"(a[13]));
}

__global__ __launch_bounds__(VP_NT) __attribute__((amdgpu_waves_per_eu(2, 2))) void lbs_vertex_pass_pipe_kernel(DevModel M, DevPose P, int B,
                                                                float* __restrict__ verts) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* A_l = smem;                                               // [2][32][A_STRIDE]
    float4* coef_l = reinterpret_cast<float4*>(A_l + 2 * 32 * A_STRIDE);     // [2][VP_NBLK][hi, lo][64]
    float* part = reinterpret_cast<float*>(coef_l + 2 * VP_NBLK * 2 * 64);   // [3][32][33]  (K halves already added)
    float* tau_l = part + 3 * 32 * 33;                               // [2][32][4]
    float4* sw_l = reinterpret_cast<float4*>(tau_l + 2 * 32 * 4);    // [32] weights of the tile's vertices
    int4* sj_l = reinterpret_cast<int4*>(sw_l + 32);                 // [32] their joints
    int* sel_l = reinterpret_cast<int*>(sj_l + 32);                  // [32] objective slot of a vertex or -1 (chained mode)
    int* live_l = sel_l + 32;                                        // [4] (2 used) chunk has a problem that is still running
    unsigned* dn_l = reinterpret_cast<unsigned*>(live_l + 4);        // [2][32] done_round words of a chunk (asynchronous fit)

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int tile = blockIdx.x;
    const int nchunks = (B + 31) >> 5;
    const int c_first = P.chunk0, nloop = nchunks - c_first;
    const bool async = P.tag != nullptr;
    const bool stream_nt = VP_NT_LOADS && async && !(P.pad_ & 1u);
    const bool store_nt = VP_NT_LOADS && async && !(P.pad_ & 2u);
    const int vbase = tile * TILE_V;
    const int nvalid_v = min(TILE_V, M.nv - vbase);                  // vertices of this tile that exist
    const float inv_scale = 1.0f / M.bs_scale;                       // power of two: exact

    if (wave < VPP_NMFMA) {
        // =========================== loader / contraction wave: coordinate plane `wave` ===========================
        // every loader wave requests its third of a chunk's operands: items 0..27 coefficient words, 28..63 transform
        // rows, 64 tau, 65 the chunk's done_round words (asynchronous fit; else tau again) - always 22 requests per wave,
        // also for a chunk index past the end (clamped), so that the counted wait below has a fixed meaning
        auto request = [&](int it, int buf) {
            const int chunk = min(c_first + it, nchunks - 1);
            const float4* csrc = P.coefH + (size_t)chunk * VP_NBLK * 2 * 64 + lane;
            const float4* asrc = reinterpret_cast<const float4*>(P.Amat + (size_t)chunk * 32 * 288) + lane;     // Bpad rows exist
            const float4* tsrc = reinterpret_cast<const float4*>(P.tau + (size_t)chunk * 32 * 4) + (lane & 31);
            float4* cdst = coef_l + buf * VP_NBLK * 2 * 64;
            float4* adst = reinterpret_cast<float4*>(A_l + buf * 32 * A_STRIDE);
            float4* tdst = reinterpret_cast<float4*>(tau_l + buf * 32 * 4);
#pragma unroll
            for (int q = 0; q < VPP_DMA_PER_WAVE; ++q) {
                const int i = wave + VPP_NMFMA * q;                  // wave-uniform
                if (i < 28) __builtin_amdgcn_global_load_lds(csrc + i * 64, cdst + i * 64, 16, 0, 0);
                else if (i < 64) __builtin_amdgcn_global_load_lds(asrc + (i - 28) * 64, adst + (i - 28) * 64, 16, 0, 0);
                // (the LDS side of a request is lane-indexed: 32 lanes for the 32-word rows)
                else if (i == 64 || !async) { if (lane < 32) __builtin_amdgcn_global_load_lds(tsrc, tdst, 16, 0, 0); }
                else if (lane < 32) __builtin_amdgcn_global_load_lds(P.done_round + (size_t)chunk * 32 + lane, dn_l + buf * 32, 4, 0, 0);
            }
        };
        request(0, 0);
        __builtin_amdgcn_sched_barrier(0);
        const float vt_init = M.vt_planes[wave * M.nv_pad + vbase + (lane & 31)] * M.bs_scale;
        float4 bh[VP_NBLK], bl[VP_NBLK];
        {
            const float4* cb = M.bs_h2 + ((size_t)(tile * 3 + wave) * VP_NBLK * 2) * 64 + lane;
#pragma unroll
            for (int g = 0; g < VP_NBLK; ++g) {
                bh[g] = stream_nt ? nt_load16(&cb[(2 * g) * 64]) : cb[(2 * g) * 64];
                if (!M.half_basis) bl[g] = stream_nt ? nt_load16(&cb[(2 * g + 1) * 64]) : cb[(2 * g + 1) * 64];
                else bl[g] = make_float4(0.f, 0.f, 0.f, 0.f);
            }
        }
        __builtin_amdgcn_sched_barrier(0);
        request(1, 1);
        __builtin_amdgcn_sched_barrier(0);
        const unsigned coef_a = (unsigned)(uintptr_t)(__attribute__((address_space(3))) void*)coef_l + 16u * (unsigned)lane;
        // D layout -> part[plane][problem][vertex]: col (vertex) = lane & 31, row (problem) = (r & 3) + 8 (r >> 2) + 4 (lane >> 5)
        const unsigned part_a = (unsigned)(uintptr_t)(__attribute__((address_space(3))) void*)part +
                                4u * (unsigned)((wave * 32 + 4 * (lane >> 5)) * 33 + (lane & 31));
        const unsigned live_a = (unsigned)(uintptr_t)(__attribute__((address_space(3))) void*)live_l;
        // Liveness of a chunk (asynchronous fit: a chunk whose 32 problems had all finished before this round is skipped):
        // the chunk's done_round words arrive with its operands (item 65, requested by the last loader wave); that wave
        // turns them into the verdict word right behind its counted wait.
        const bool live_wave = wave == (65 % VPP_NMFMA);
        const unsigned dn_a = (unsigned)(uintptr_t)(__attribute__((address_space(3))) void*)dn_l + 4u * (unsigned)(lane & 31);
        __syncthreads();                                             // (0) tables written by the workers, first liveness word
        for (int it = 0; it < nloop; ++it) {
            const int buf = it & 1;
#ifdef MVFIT_TIMING
            const long long t_it = clock64();               // timeline of the third chunk (steady state), tests/vp_timeline.py
#define VPP_T(k_) do { if (it == 2) VP_T(k_, t_it); } while (0)
#else
#define VPP_T(k_) do { } while (0)
#endif
            // the operands of this chunk were requested two iterations ago (the first two: up front); only the request of
            // the NEXT chunk - the newest 22 loads of this wave - may still be in flight
            asm volatile("s_waitcnt vmcnt(22)" ::: "memory");
            VPP_T(0);
            if (live_wave) {
                bool lv = true;
                if (async) {
                    unsigned d;
                    asm volatile("ds_read_b32 %0, %1\n\ts_waitcnt lgkmcnt(0)" : "=v"(d) : "v"(dn_a + 128u * (unsigned)buf));
                    const int b = (c_first + it) * 32 + lane;
                    lv = __ballot(lane < 32 && b < B && d > P.round) != 0ull;
                }
                if (lane == 0) lds_write4_nowait(live_a + 4u * (unsigned)buf, __builtin_bit_cast(float, lv ? 1 : 0));
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            }
            __syncthreads();                                         // (1) operands visible; partials of the last chunk consumed
            VPP_T(1);
            int live;
            asm volatile("ds_read_b32 %0, %1\n\ts_waitcnt lgkmcnt(0)" : "=v"(live) : "v"((unsigned)(uintptr_t)(__attribute__((address_space(3))) void*)(live_l + buf)));
            live = __builtin_amdgcn_readfirstlane(live);
            if (live) {
                // ---- contraction: K half 0 (v_template in the accumulator), K half 1; small products first ----
                floatx16 acc0, acc1;
#pragma unroll
                for (int r = 0; r < 16; ++r) { acc0[r] = vt_init; acc1[r] = 0.f; }
                const unsigned ca = coef_a + (unsigned)buf * (VP_NBLK * 2 * 64 * 16);
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    f32x4v aw[14];                                   // (hi, lo) words of 7 blocks
#pragma unroll
                    for (int q = 0; q < 14; ++q) aw[q] = lds_read16_nowait(ca + (unsigned)((14 * h + q) * 64 * 16));
                    lds_wait14(aw);
#pragma unroll
                    for (int g = 0; g < VP_BPW; ++g) {
                        const half8 Ah = __builtin_bit_cast(half8, aw[2 * g]), Al = __builtin_bit_cast(half8, aw[2 * g + 1]);
                        const half8 Bh = __builtin_bit_cast(half8, bh[VP_BPW * h + g]), Bl = __builtin_bit_cast(half8, bl[VP_BPW * h + g]);
                        if (h == 0) {
                            acc0 = __builtin_amdgcn_mfma_f32_32x32x16_f16(Al, Bh, acc0, 0, 0, 0);
                            acc0 = __builtin_amdgcn_mfma_f32_32x32x16_f16(Ah, Bl, acc0, 0, 0, 0);
                            acc0 = __builtin_amdgcn_mfma_f32_32x32x16_f16(Ah, Bh, acc0, 0, 0, 0);
                        } else {
                            acc1 = __builtin_amdgcn_mfma_f32_32x32x16_f16(Al, Bh, acc1, 0, 0, 0);
                            acc1 = __builtin_amdgcn_mfma_f32_32x32x16_f16(Ah, Bl, acc1, 0, 0, 0);
                            acc1 = __builtin_amdgcn_mfma_f32_32x32x16_f16(Ah, Bh, acc1, 0, 0, 0);
                        }
                    }
                }
                VPP_T(2);
#pragma unroll
                for (int r = 0; r < 16; ++r)
                    lds_write4_nowait(part_a + 4u * (unsigned)(((r & 3) + 8 * (r >> 2)) * 33), acc0[r] + acc1[r]);
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                VPP_T(3);
                __syncthreads();                                     // (2) partials published; this chunk's operand buffer is free
                VPP_T(4);
            }
            request(it + 2, buf);                                    // the chunk after next, into the buffer just released
            VPP_T(5);
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");             // no request may outlive the workgroup's LDS
        return;
    }

    // ======================================= worker waves: 320 threads, 512 items =======================================
    const int wt = tid - 64 * VPP_NMFMA;                             // 0..319
    const int w_vp2 = wt & 15, w_bb0 = wt >> 4;                      // item 0: problem 0..19; item 1: problem 20..31
    const bool w_two = wt < (512 - VPP_NWORK);
    if (wt < 32) sw_l[wt] = M.wsp_w[(size_t)vbase + wt];
    else if (wt < 64) sj_l[wt - 32] = M.wsp_j[(size_t)vbase + wt - 32];
    else if (wt < 96) sel_l[wt - 64] = -1;
    if (!async) {                                                    // objective slots of this tile's vertices (side outputs)
        wave_lds_fence();
        if (wave == VPP_NMFMA + 1) {                                 // the wave that wrote the -1s
            const int s0 = M.tile_sel_start[tile], s1 = M.tile_sel_start[tile + 1];
            if (lane < s1 - s0) sel_l[M.tile_sel_local[s0 + lane]] = M.tile_sel_slot[s0 + lane];
        }
    }
    __syncthreads();                                                 // (0)
    for (int it = 0; it < nloop; ++it) {
        const int chunk = c_first + it, b0 = chunk * 32, buf = it & 1;
#ifdef MVFIT_TIMING
        const long long t_it = clock64();
#endif
        __syncthreads();                                             // (1)
        VPP_T(1);
        const bool live = live_l[buf] != 0;                          // uniform
        if (async && blockIdx.x == 0 && wt == 0) atomicAdd(P.stats + (live ? 0 : 1), 1u);      // chunk passes run / skipped
        if (!live) continue;
        // ---- skinning blend of this chunk's items, while the planes are contracted ----
        const float* A_c = A_l + buf * 32 * A_STRIDE;
        float tr0[3][2][4], tr1[3][2][4];
        vp_blend_zero(tr0);
        vp_blend_zero(tr1);
        {
            const float4 swa = sw_l[2 * w_vp2], swb = sw_l[2 * w_vp2 + 1];
            const int4 sja = sj_l[2 * w_vp2], sjb = sj_l[2 * w_vp2 + 1];
            vp_blend_pairs(tr0, 0, A_c + w_bb0 * A_STRIDE, swa, sja);
            vp_blend_pairs(tr0, 1, A_c + w_bb0 * A_STRIDE, swb, sjb);
            if (w_two) {
                vp_blend_pairs(tr1, 0, A_c + (w_bb0 + 20) * A_STRIDE, swa, sja);
                vp_blend_pairs(tr1, 1, A_c + (w_bb0 + 20) * A_STRIDE, swb, sjb);
            }
        }
        const float4 ta = *reinterpret_cast<const float4*>(tau_l + buf * 32 * 4 + w_bb0 * 4);
        const float4 tb = *reinterpret_cast<const float4*>(tau_l + buf * 32 * 4 + (w_two ? w_bb0 + 20 : w_bb0) * 4);
        VPP_T(2);
        __syncthreads();                                             // (2) partials published
        VPP_T(4);
        // ---- v_posed (K halves added by the contraction wave; scale undone), T applied, + transl, store ----
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            if (e == 1 && !w_two) break;
            const int bb = e ? w_bb0 + 20 : w_bb0;
            const float (&tr)[3][2][4] = e ? tr1 : tr0;
            const float tau3[3] = {e ? tb.x : ta.x, e ? tb.y : ta.y, e ? tb.z : ta.z};
            float o[6];
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const int v = 2 * w_vp2 + i;
                float vp[3];
#pragma unroll
                for (int k = 0; k < 3; ++k) vp[k] = part[(k * 32 + bb) * 33 + v] * inv_scale;
                float xs[3];
#pragma unroll
                for (int k = 0; k < 3; ++k)
                    xs[k] = fmaf(tr[k][i][0], vp[0], fmaf(tr[k][i][1], vp[1], fmaf(tr[k][i][2], vp[2], tr[k][i][3])));
                if (!async) {                                        // side outputs of the chained mode (objective vertices only)
                    const int slot = sel_l[v];
                    if (slot >= 0 && b0 + bb < B) {
#pragma unroll
                        for (int k = 0; k < 3; ++k) {
                            P.vposed_sel[(size_t)(b0 + bb) * NC_MAX + 3 * slot + k] = vp[k];
                            P.xs_sel[(size_t)(b0 + bb) * NC_MAX + 3 * slot + k] = xs[k];
                        }
                    }
                }
#pragma unroll
                for (int k = 0; k < 3; ++k) o[3 * i + k] = xs[k] + tau3[k];
            }
            if (b0 + bb < B) {
                // 24 contiguous bytes (vertices 2 vp2, 2 vp2 + 1), 8-byte aligned (even vertex count, checked at launch)
                float* dst = verts + ((size_t)(b0 + bb) * M.nv + vbase + 2 * w_vp2) * 3;
                const int nv_ok = nvalid_v - 2 * w_vp2;              // vertices of this pair that exist
                if (nv_ok >= 2) {
                    const f32x2 q0 = {o[0], o[1]}, q1 = {o[2], o[3]}, q2 = {o[4], o[5]};
                    if (store_nt) {
                        __builtin_nontemporal_store(q0, reinterpret_cast<f32x2*>(dst));
                        __builtin_nontemporal_store(q1, reinterpret_cast<f32x2*>(dst + 2));
                        __builtin_nontemporal_store(q2, reinterpret_cast<f32x2*>(dst + 4));
                    } else {
                        *reinterpret_cast<f32x2*>(dst) = q0; *reinterpret_cast<f32x2*>(dst + 2) = q1; *reinterpret_cast<f32x2*>(dst + 4) = q2;
                    }
                } else if (nv_ok == 1) {
                    dst[0] = o[0]; dst[1] = o[1]; dst[2] = o[2];
                }
            }
        }
        VPP_T(5);
    }
#ifdef MVFIT_TIMING
    if (blockIdx.x == 5 && threadIdx.x == 256) g_vp[7] += 1;
#endif
}

// compile-time loop: f(integral_constant<int, 0>) ... f(integral_constant<int, N - 1>) (builtin arguments that must be constants)
template <int... Ks, typename F>
__device__ __forceinline__ void static_for(std::integer_sequence<int, Ks...>, F&& f) { (f(std::integral_constant<int, Ks>{}), ...); }

// ---------------------------------------------------------------------------------------------------------
// Resident pass of the asynchronous fit: ONE launch per (sub-batch) fit instead of a gate + a pass launch per closure round.
//
// The per-round launches above re-stream the 18.2 MB basis every round (379 times per 32-frame fit) and pay launch, ramp
// and teardown around ~3 us of work.  Here a workgroup owns TPW vertex tiles for the whole fit: the tiles' split-fp16
// basis is loaded ONCE into registers (56 VGPRs per contraction chain = tile x coordinate plane x K half, the chains of
// lbs_vertex_pass_split_kernel), and the workgroup then serves closure round after closure round from the operand ring:
//   * wave 7 polls the round's ring tags (relaxed agent-scope = sc1 loads, s_sleep between polls: one idle wave per
//     workgroup, the form the guide's polling-cost row asks for) while the other waves sleep at the barrier; the verdict
//     (go / all problems finished / timed out) and the mask of live 32-problem chunks go through LDS;
//   * the operands of a chunk (28 KiB of split-fp16 coefficient words, 36 KiB of skinning transforms, translations) come
//     as direct global -> LDS loads with sc1: the optimiser wrote them with sc1 (write-through) stores and drained them
//     before the tag, so sc1 on both sides is the whole hand-off - no acquire fence, nothing invalidated under the
//     optimiser workgroups of the same XCD.  The NEXT live chunk's operands are requested while this chunk is blended and
//     stored: as soon as every contraction has read this chunk's coefficients, the transforms into the other of two
//     buffers, the coefficients into their single one.  The buffers are separate __shared__ objects, so the compiler's
//     wait-count pass knows which LDS accesses an in-flight request can touch (one dynamic array would make it wait for
//     the request at the next LDS instruction); the barriers inside a chunk are bare s_barrier + lgkmcnt waits for the
//     same reason (__syncthreads' fence waits for every outstanding request);
//   * the 6 * TPW contraction chains are spread so that every SIMD carries the same number (TPW = 2: waves 0-3 two chains,
//     waves 4-7 one; 21 dependent MFMAs each, the association of the per-round kernels: bit-identical vertices); all eight
//     waves blend (4-pair skinning table), apply and store their (vertex pair, problem) items STRAIGHT from registers
//     (24 contiguous bytes per item, 384-byte runs per problem) - no staging of the output, two barriers per chunk; the
//     last tile's stores of a chunk are issued behind the chunk's closing barrier, so that the wait for the next chunk's
//     operands never waits for fresh store acknowledgements;
//   * back-pressure: the workgroup publishes the number of rounds whose operands it has read in its OWN word
//     (ResidentArgs::wg_round); the optimiser takes the minimum over the words when its cached copy does not cover
//     `round - nslots` (a few times per fit) - no atomics, no contention.
// Per closure round the pass now moves 84,712 bytes per problem + the operands; the basis crosses the memory system once
// per fit.  Grid = ceil(ntiles / TPW) workgroups that must all be resident next to the optimiser's (one CU each): the host
// picks TPW from the CU count (fit_plan.cpp: resident_form).  Vertices bit-identical to the per-round kernels
// (tests/test_gpu_async.py).  mvfit_profile: every workgroup logs {operands seen, stores drained} per round (wall clock).
// ---------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void wg_barrier_lds() {           // workgroup barrier that orders LDS traffic only (see above)
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
}

// ---- the polling wave of a resident workgroup (both resident kernels): wait for the operands of closure round r ----
// Every problem of the sub-batch has published round r (tag >= r + 1) or finished before it (done_round <= r).  Verdicts:
//   VR_GO      serve the round: ctl[1] = mask of the 32-problem chunks with a live problem;
//   VR_DONE    every problem finished before this round: the fit is over;
//   VR_TIMEOUT the operands did not arrive within 20 ms (wall clock): this workgroup leaves the launch;
//   VR_LOST    a live problem's slot already holds a LATER round (this workgroup fell a whole ring behind - it was not resident
//              in time, or the optimiser gave up waiting for it): the round is skipped, nothing is computed from operands of
//              another round and nothing is stored; a workgroup that starts after the fit has ended runs through its rounds
//              this way in a poll each instead of replaying them from stale slots.
// Degradation is reported by EVERY workgroup (round 6; before, only workgroup 0 counted): stats[2] = the largest number of
// (problem, round) operand sets any ONE workgroup lost (atomicMax of the workgroup's running total; all workgroups that keep
// up report 0), stats[3] += 1 for every workgroup that timed out.  stats[0] / [1] (chunk passes run / skipped) stay
// workgroup 0's: they describe the schedule, not a fault.
enum : unsigned { VR_GO = 1u, VR_DONE = 2u, VR_TIMEOUT = 3u, VR_LOST = 4u };
__device__ __forceinline__ void resident_poll(const ResidentArgs& RA, unsigned r, unsigned slot, unsigned nch, int lane, int wg,
                                              unsigned* ctl, unsigned& lost_total) {
    const unsigned want = r + 1u;
    const unsigned* tg = RA.tag + (size_t)slot * RA.rb;
    const unsigned* dn = RA.done_round + RA.b_lo;
    unsigned verdict = VR_GO, missed = 0u;
    unsigned rows_live[4] = {0u, 0u, 0u, 0u};                  // per 32-row chunk: the rows whose problem evaluates round r
    const long long t0 = wall_clock64();
    for (;;) {
        bool ok = true;
        missed = 0u;
#pragma unroll
        for (int j = 0; j < 2; ++j) {                          // (at most 128 rows: kResidentMaxB, checked by the host)
            const int p = lane + 64 * j;
            bool live = false;
            if (p < RA.n) {
                const unsigned t = __hip_atomic_load(tg + p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                const unsigned d = __hip_atomic_load(dn + p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                live = d > r;                                  // the row's problem evaluates (or evaluated) closure round r
                ok = ok && (t >= want || !live);               // (a larger tag: a later round already overwrote the slot)
                if (live && t > want) ++missed;
            }
            const unsigned long long bal = __ballot(live);
            rows_live[2 * j] = (unsigned)bal; rows_live[2 * j + 1] = (unsigned)(bal >> 32);
        }
        if (__all(ok)) break;
        if (wall_clock64() - t0 > 2000000) { verdict = VR_TIMEOUT; break; }            // 20 ms at 100 MHz
        __builtin_amdgcn_s_sleep(8);                              // (round 6: 8 instead of 32 - measured in round 5: the round span 4.74 -> 4.6 us, closures/s unchanged)
    }
    unsigned mask = 0u;
    for (unsigned c = 0; c < nch; ++c) mask |= rows_live[c & 3u] != 0u ? (1u << c) : 0u;
    if (verdict == VR_GO && mask == 0u) verdict = VR_DONE;     // every problem finished before this round: the fit is over
    if (verdict == VR_GO && __ballot(missed != 0u)) {          // operands overwritten before this workgroup read them
        unsigned msum = missed;
        for (int o = 32; o; o >>= 1) msum += __shfl_xor(msum, o);
        lost_total += msum;
        verdict = VR_LOST;
        if (lane == 0) atomicMax(RA.stats + 2, lost_total);
    }
    if (lane == 0) {
        ctl[0] = verdict; ctl[1] = mask;
        const long long ts = wall_clock64();
        ctl[2] = (unsigned)ts; ctl[3] = (unsigned)((unsigned long long)ts >> 32);
        // the live rows of every chunk: a dead row of a live chunk (its problem finished earlier) is not stored - its ring slot
        // holds whatever an earlier round, or an earlier fit, left there (round 6: the destination is the slot's own problem word)
        ctl[4] = rows_live[0]; ctl[5] = rows_live[1]; ctl[6] = rows_live[2]; ctl[7] = rows_live[3];
        if (wg == 0 && verdict == VR_GO) {
            atomicAdd(RA.stats + 0, (unsigned)__popc(mask));
            if (nch > (unsigned)__popc(mask)) atomicAdd(RA.stats + 1, nch - (unsigned)__popc(mask));
        }
        if (verdict == VR_TIMEOUT) atomicAdd(RA.stats + 3, 1u);
    }
}

template <int TPW, bool HALF>
__global__ __launch_bounds__(VP_NT) __attribute__((amdgpu_waves_per_eu(2, 2))) void lbs_vertex_pass_resident_kernel(DevModel M, ResidentArgs RA) {
    // separate LDS objects (alias information for the wait-count pass, see above)
    // (element types = access widths, and every access below indexes the array itself: an access through a generic
    // float* loses the alias information and waits for every request in flight)
    __shared__ __attribute__((aligned(16))) f32x4 A_0[32 * A_STRIDE / 4];      // skinning transforms of a chunk, two buffers
    __shared__ __attribute__((aligned(16))) f32x4 A_1[32 * A_STRIDE / 4];
    __shared__ __attribute__((aligned(16))) f32x4 coef_l[VP_NBLK * 2 * 64];    // [VP_NBLK][hi, lo][64 lanes] A operands of a chunk
    __shared__ __attribute__((aligned(16))) f32x4 tau_0[32];
    __shared__ __attribute__((aligned(16))) f32x4 tau_1[32];
    __shared__ float part[TPW * 2 * 3 * 32 * 33];                             // [TPW][2 K-halves][3][32][33]
    __shared__ f32x4 sw_l[TPW * 32];                                          // 4-pair skinning table of the tiles' vertices
    __shared__ i32x4 sj_l[TPW * 32];
    __shared__ float vt_l[TPW * VP_NT];                                       // v_template rows of the chains (accumulator start)
    __shared__ unsigned ctl[8];                                               // verdict, live-chunk mask, stamp (2 words)

    const int tid_k = threadIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane(tid_k >> 6);
    const int wg = blockIdx.x;
    const bool store_nt = VP_NT_LOADS && !(RA.flags & 2u);
    const float inv_scale = 1.0f / M.bs_scale;            // power of two: exact
    const unsigned nch = (unsigned)(RA.n + 31) >> 5;
    // contraction chains: id = K-half * 3 TPW + tile * 3 + plane; every SIMD (wave & 3) carries 6 TPW / 4 of them
    const int nchain = TPW == 1 ? (wave < 6 ? 1 : 0) : (wave < 4 ? 2 : 1);
    const int chain0 = TPW == 1 ? wave : (wave < 4 ? 2 * wave : wave + 4);
    const int kh_w = chain0 / (3 * TPW);                   // all chains of a wave are of one K half

    // ---- once per fit: the chains' basis (B operands of the contraction), v_template, skinning tables ----
    float4 bh[TPW][VP_BPW], bl[HALF ? 1 : TPW][HALF ? 1 : VP_BPW];       // HALF (configs[4]): only the hi halves of the basis are read
    int ch_t[TPW], ch_kc[TPW];
#pragma unroll
    for (int s = 0; s < TPW; ++s) {
        const int id = min(chain0 + s, 6 * TPW - 1);
        const int rem = id - (id / (3 * TPW)) * (3 * TPW);
        ch_t[s] = rem / 3; ch_kc[s] = rem - 3 * ch_t[s];
        const int tile = min(wg * TPW + ch_t[s], M.ntiles - 1);           // (a tile past the end is never stored)
        vt_l[s * VP_NT + tid_k] = 0.f;
        if (s < nchain) {
            const int lane = tid_k & 63;
            if (kh_w == 0) vt_l[s * VP_NT + tid_k] = M.vt_planes[ch_kc[s] * M.nv_pad + tile * TILE_V + (lane & 31)] * M.bs_scale;
            const float4* cb = M.bs_h2 + ((size_t)((tile * 3 + ch_kc[s]) * VP_NBLK + kh_w * VP_BPW) * 2) * 64 + lane;
#pragma unroll
            for (int g = 0; g < VP_BPW; ++g) {
                bh[s][g] = nt_load16(&cb[(2 * g) * 64]);
                if (!HALF) bl[s][g] = nt_load16(&cb[(2 * g + 1) * 64]);
            }
        }
    }
#pragma unroll
    for (int t = 0; t < TPW; ++t) {
        const int tile = min(wg * TPW + t, M.ntiles - 1);
        if (tid_k < 32) sw_l[t * 32 + tid_k] = __builtin_bit_cast(f32x4, M.wsp_w[(size_t)tile * TILE_V + tid_k]);
        else if (tid_k < 64) sj_l[t * 32 + tid_k - 32] = __builtin_bit_cast(i32x4, M.wsp_j[(size_t)tile * TILE_V + tid_k - 32]);
    }
    __syncthreads();
    bool pair_same[TPW];                                         // the two vertices of this thread's pair hang on the same joints
#pragma unroll
    for (int t = 0; t < TPW; ++t) {
        const i32x4 a = sj_l[t * 32 + 2 * (tid_k & 15)], b = sj_l[t * 32 + 2 * (tid_k & 15) + 1];
        pair_same[t] = a.x == b.x && a.y == b.y && a.z == b.z && a.w == b.w;
    }

    // requests of a chunk's operands: direct global -> LDS, sc1; spread over the eight waves (A: 36 x 1 KiB, coefficients 28);
    // Q = the buffer the transforms go to (compile-time: the destination is a named LDS object)
    auto request_A = [&](auto Q_, unsigned slot, unsigned c, int lane) {
        constexpr int Q = decltype(Q_)::value;
        const float4* asrc = reinterpret_cast<const float4*>(RA.Amat) + ((size_t)slot * RA.rb + c * 32u) * 72 + lane;
        static_assert(A_STRIDE == 288, "a chunk's transforms are one linear 36 KiB copy");
        // consecutive KiB per wave (waves 0-3: five, waves 4-7: four); the instruction offset (0 .. 3 KiB) moves BOTH addresses, so
        // four requests share one global address and one M0 - a request is then one or two instructions, not eight
        const int a0 = wave < 4 ? 5 * wave : 4 * wave + 4;
        const float4* g = asrc + a0 * 64;
        static_for(std::make_integer_sequence<int, 5>{}, [&](auto K_) {
            constexpr int k = decltype(K_)::value;
            if (k < 4 || wave < 4) {                                             // (uniform)
                if constexpr (Q == 0) __builtin_amdgcn_global_load_lds(g + (k >> 2) * 256, &A_0[(a0 + (k & ~3)) * 64], 16, (k & 3) * 1024, /*aux = sc1*/ 16);
                else __builtin_amdgcn_global_load_lds(g + (k >> 2) * 256, &A_1[(a0 + (k & ~3)) * 64], 16, (k & 3) * 1024, 16);
            }
        });
        if (wave == 7 && lane < 32) {
            const float4* tsrc = reinterpret_cast<const float4*>(RA.tau) + ((size_t)slot * RA.rb + c * 32u) + lane;
            if constexpr (Q == 0) __builtin_amdgcn_global_load_lds(tsrc, &tau_0[0], 16, 0, 16);
            else __builtin_amdgcn_global_load_lds(tsrc, &tau_1[0], 16, 0, 16);
        }
    };
    auto request_coef = [&](unsigned slot, unsigned c, int lane) {
        const float4* csrc = RA.coefH + ((size_t)slot * ((unsigned)RA.rb >> 5) + c) * (VP_NBLK * 2 * 64) + lane;
        static_assert(VP_NBLK * 2 == 28, "three KiB per wave 0-3, four per wave 4-7 (which carry one chain)");
        const int c0 = wave < 4 ? 3 * wave : 4 * wave - 4;
        const float4* g = csrc + c0 * 64;
        static_for(std::make_integer_sequence<int, 4>{}, [&](auto K_) {
            constexpr int k = decltype(K_)::value;
            if (k < 3 || wave >= 4) __builtin_amdgcn_global_load_lds(g, &coef_l[c0 * 64], 16, k * 1024, 16);
        });
    };

    // a (vertex pair, problem) item's finished vertices, kept in registers until their stores are issued
    struct Pending { float o[6]; float* dst; int nv_ok; };
    auto issue_stores = [&](const Pending& q) {
        if (q.nv_ok >= 2) {
            // 24 contiguous bytes (vertices 2 vp2, 2 vp2 + 1), 8-byte aligned (even vertex count, checked by the host)
            const f32x2 q0 = {q.o[0], q.o[1]}, q1 = {q.o[2], q.o[3]}, q2 = {q.o[4], q.o[5]};
            if (store_nt) {
                __builtin_nontemporal_store(q0, reinterpret_cast<f32x2*>(q.dst));
                __builtin_nontemporal_store(q1, reinterpret_cast<f32x2*>(q.dst + 2));
                __builtin_nontemporal_store(q2, reinterpret_cast<f32x2*>(q.dst + 4));
            } else {
                *reinterpret_cast<f32x2*>(q.dst) = q0; *reinterpret_cast<f32x2*>(q.dst + 2) = q1; *reinterpret_cast<f32x2*>(q.dst + 4) = q2;
            }
        } else if (q.nv_ok == 1) {
            q.dst[0] = q.o[0]; q.dst[1] = q.o[1]; q.dst[2] = q.o[2];
        }
    };

    unsigned lost_total = 0u;                                   // (polling wave) operand sets this workgroup lost so far
    for (unsigned r = 0; r < RA.max_rounds; ++r) {
        const unsigned slot = r % (unsigned)RA.nslots;
        // ---- wave 7: wait for the operands of closure round r (every problem: published, or finished before r) ----
        if (wave == 7) resident_poll(RA, r, slot, nch, tid_k & 63, wg, ctl, lost_total);
        __syncthreads();
        const unsigned verdict = ctl[0];
        unsigned mask = ctl[1];
        if (verdict == VR_LOST) {                              // uniform: skip the round (see resident_poll)
            __syncthreads();                                   // (every wave has read ctl before wave 7 polls the next round)
            if (tid_k == 0) __hip_atomic_store(RA.wg_round + wg, r + 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            continue;
        }
        if (verdict != VR_GO) break;                           // uniform
        float* vout = (RA.capture_verts && (int)r == RA.capture_round) ? RA.capture_verts : RA.verts;

        // ---- the round's first live chunk: nothing to overlap its operands with ----
        unsigned c = (unsigned)__builtin_ctz(mask);
        mask &= mask - 1u;
        {
            const int lane = tid_k & 63;
            request_A(std::integral_constant<int, 0>{}, slot, c, lane);
            request_coef(slot, c, lane);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            wg_barrier_lds();
        }
        unsigned par = 0u;
        // one chunk out of the buffers of parity P (compile-time: the buffers are distinct LDS objects)
        auto chunk = [&](auto P_, unsigned c, int cn) {
            constexpr int P = decltype(P_)::value;
            auto A_row = [&](int idx) -> f32x4 { if constexpr (P == 0) return A_0[idx]; else return A_1[idx]; };   // 16-byte words
            // opaque copy of the thread index: keeps the compiler from hoisting every tid-derived address of the chunk out of
            // the round loop (the basis already holds 56 registers per chain; hoisted addresses spill)
            int tid = tid_k;
            asm volatile("" : "+v"(tid));
            const int lane = tid & 63, vp2 = tid & 15, bb = tid >> 4;
#ifdef MVFIT_TIMING
            const long long t_ch = clock64();                  // timeline of a chunk in buffer 1 (steady state), tests/vp_resident_timeline.py
#define VPR_T(k_) do { if (P == 1) VP_T(k_, t_ch); } while (0)
#else
#define VPR_T(k_) do { } while (0)
#endif
            // (c) blendshape contraction: this wave's chains (one K half; plane, tile per chain); small products first.  The
            //     chunk's A operands are read once per block and feed the chains' independent accumulators
            // (straight-line code per chain count: a per-MFMA `if (s < nchain)` costs accumulator copies)
            auto contract = [&](auto NC_) {
                constexpr int NC = decltype(NC_)::value;
                floatx16 acc[NC];
#pragma unroll
                for (int s = 0; s < NC; ++s)
#pragma unroll
                    for (int q = 0; q < 16; ++q) acc[s][q] = vt_l[s * VP_NT + tid];
                const int cl = (kh_w * VP_BPW * 2) * 64 + lane;
#pragma unroll
                for (int g = 0; g < VP_BPW; ++g) {
                    const half8 Ah = __builtin_bit_cast(half8, coef_l[cl + (2 * g) * 64]), Al = __builtin_bit_cast(half8, coef_l[cl + (2 * g + 1) * 64]);
#pragma unroll
                    for (int s = 0; s < NC; ++s) {
                        const half8 Bh = __builtin_bit_cast(half8, bh[s][g]);
                        acc[s] = __builtin_amdgcn_mfma_f32_32x32x16_f16(Al, Bh, acc[s], 0, 0, 0);
                        if (!HALF) acc[s] = __builtin_amdgcn_mfma_f32_32x32x16_f16(Ah, __builtin_bit_cast(half8, bl[HALF ? 0 : s][HALF ? 0 : g]), acc[s], 0, 0, 0);
                        acc[s] = __builtin_amdgcn_mfma_f32_32x32x16_f16(Ah, Bh, acc[s], 0, 0, 0);
                    }
                    // one block's operands in flight at a time (registers; reading block g + 1 under block g's MFMAs was
                    // measured: no gain - the one-chain waves of the same SIMDs set the phase's length)
                    if (NC > 1) __builtin_amdgcn_sched_barrier(0);
                }
#pragma unroll
                for (int s = 0; s < NC; ++s) {
                    // MFMA D layout -> part[tile][K half][plane][problem][33]: col (vertex) = lane & 31,
                    // row (problem) = (r & 3) + 8 (r >> 2) + 4 (lane >> 5)
                    const int p0 = (((ch_t[s] * 2 + kh_w) * 3 + ch_kc[s]) * 32 + 4 * (lane >> 5)) * 33 + (lane & 31);
#pragma unroll
                    for (int q = 0; q < 16; ++q) part[p0 + ((q & 3) + 8 * (q >> 2)) * 33] = acc[s][q];
                }
            };
            if (nchain == TPW) contract(std::integral_constant<int, TPW>{});
            else if (TPW > 1 && nchain == 1) contract(std::integral_constant<int, 1>{});
            VPR_T(0);
            wg_barrier_lds();                                  // partials published; every chain has read the coefficients
            VPR_T(1);
            // (d) the next live chunk's operands: transforms into the other buffer, coefficient words into the buffer just
            //     released.  (Not earlier: no request is in flight while the partials are written - the wait-count pass
            //     loses the alias information of some of those LDS stores and would wait for the requests there)
            if (cn >= 0) {
                request_A(std::integral_constant<int, 1 - P>{}, slot, (unsigned)cn, lane);
                request_coef(slot, (unsigned)cn, lane);
            }
            __builtin_amdgcn_sched_barrier(0);
            VPR_T(2);
            // (e) all waves: skinning blend (lbs.py:209-213), K halves combined in a fixed order, scale undone, T applied,
            //     "+ transl"; stores straight from registers (the last tile's: behind the closing barrier)
            const bool b_ok = ((ctl[4 + c] >> bb) & 1u) != 0u;     // (the row's problem evaluates this round)
            f32x4 tq;
            if constexpr (P == 0) tq = tau_0[bb]; else tq = tau_1[bb];
            const float tau3[3] = {tq.x, tq.y, tq.z};
            // the problem this ring row held in this round (the translation word's spare lane; rows take new problems from the
            // launch's work queue when theirs has finished - fit_kernels.hip: fit_persistent_kernel)
            // (through a float rvalue: __builtin_bit_cast applied to the swizzle expression `tq.w` itself reads the VECTOR's first
            // four bytes - element x - with this compiler, ROCm 7.2 clang; found as a memory fault, confirmed on a ten-line kernel)
            const float tq_w = tq.w;
            const int b_me = __builtin_bit_cast(int, tq_w);
            Pending last;
#pragma unroll
            for (int t = 0; t < TPW; ++t) {
                const int tile = wg * TPW + t;
                if (tile >= M.ntiles) break;                   // uniform
                // per vertex of the item: T[k][:] = sum over its 4 (weight, joint) pairs, ascending joint order - the non-zero
                // products of the dense blend in the same order (vp_blend_pairs) -, then v_posed from the two K halves (fixed
                // order, scale undone), T applied, "+ transl".  One vertex at a time, two pairs = 6 transform rows in flight:
                // the tiles' basis sits in registers next to this
                const int pt = t * (2 * 3 * 32 * 33);
                Pending cur;
                // (round 6: the pair's second vertex keeps the first one's twelve transform rows when it hangs on the same four
                // joints - 93 % of the pairs -: half the LDS gathers of the blend, the same products in the same order)
                f32x4 rows[4][3];
#pragma unroll
                for (int i = 0; i < 2; ++i) {
                    const f32x4 spw = sw_l[t * 32 + 2 * vp2 + i];
                    const i32x4 spj = sj_l[t * 32 + 2 * vp2 + i];
                    const float wq[4] = {spw.x, spw.y, spw.z, spw.w};
                    const int jq[4] = {spj.x, spj.y, spj.z, spj.w};
                    float tr[3][4];
#pragma unroll
                    for (int k = 0; k < 3; ++k)
#pragma unroll
                        for (int e = 0; e < 4; ++e) tr[k][e] = 0.f;
                    if (i == 0 || !pair_same[t]) {
#pragma unroll
                        for (int u = 0; u < 4; ++u)
#pragma unroll
                            for (int k = 0; k < 3; ++k) rows[u][k] = A_row(bb * (A_STRIDE / 4) + jq[u] * 3 + k);
                    }
#pragma unroll
                    for (int u = 0; u < 4; ++u)
#pragma unroll
                        for (int k = 0; k < 3; ++k) {
                            const f32x4 a = rows[u][k];
                            tr[k][0] = fmaf(wq[u], a.x, tr[k][0]);
                            tr[k][1] = fmaf(wq[u], a.y, tr[k][1]);
                            tr[k][2] = fmaf(wq[u], a.z, tr[k][2]);
                            tr[k][3] = fmaf(wq[u], a.w, tr[k][3]);
                        }
                    __builtin_amdgcn_sched_barrier(0);
                    const int v = 2 * vp2 + i;
                    float vp[3];
#pragma unroll
                    for (int k = 0; k < 3; ++k) {
                        float sm = part[pt + ((0 * 3 + k) * 32 + bb) * 33 + v];
                        sm += part[pt + ((1 * 3 + k) * 32 + bb) * 33 + v];
                        vp[k] = sm * inv_scale;
                    }
#pragma unroll
                    for (int k = 0; k < 3; ++k)
                        cur.o[3 * i + k] = fmaf(tr[k][0], vp[0], fmaf(tr[k][1], vp[1], fmaf(tr[k][2], vp[2], tr[k][3]))) + tau3[k];
                    __builtin_amdgcn_sched_barrier(0);
                }
                if (t + 1 < TPW && tile + 1 < M.ntiles) {
                    const int vbase = tile * TILE_V;
                    cur.dst = vout + ((size_t)b_me * M.nv + vbase + 2 * vp2) * 3;
                    cur.nv_ok = b_ok ? min(TILE_V, M.nv - vbase) - 2 * vp2 : 0;
                    issue_stores(cur);
                } else {
#pragma unroll
                    for (int q = 0; q < 6; ++q) last.o[q] = cur.o[q];
                }
                __builtin_amdgcn_sched_barrier(0);
                if (t == 0) VPR_T(3);
            }
            VPR_T(4);
            // (f) the next chunk's operands have landed (this wave's requests; the stores issued above are a tile old); the
            //     last tile's stores go out BEHIND the closing barrier: the wait never waits for fresh store acknowledgements
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            VPR_T(5);
            wg_barrier_lds();
            VPR_T(6);
#ifdef MVFIT_TIMING
            if (P == 1 && blockIdx.x == 5 && (tid_k & 255) == 0) g_vp[7 + (tid_k >> 8) * 8] += 1;
#endif
            {   // (address and validity recomputed here: three registers less across the barrier)
                int t2 = tid_k;
                asm volatile("" : "+v"(t2));
                const int tile = min(wg * TPW + TPW - 1, M.ntiles - 1), vbase = tile * TILE_V, vq = t2 & 15;
                last.dst = vout + ((size_t)b_me * M.nv + vbase + 2 * vq) * 3;      // (b_me, b_ok: kept across the barrier)
                last.nv_ok = b_ok ? min(TILE_V, M.nv - vbase) - 2 * vq : 0;      // (b_ok: read before the barrier - wave 7 may be polling the next round by now)
                issue_stores(last);
            }
        };
        for (;;) {
            const int cn = mask ? __builtin_ctz(mask) : -1;
            if (par == 0u) chunk(std::integral_constant<int, 0>{}, c, cn);
            else chunk(std::integral_constant<int, 1>{}, c, cn);
            if (cn < 0) break;
            // the first chunk of a round always lands in buffer 0 (see above): parity restarts every round
            mask &= mask - 1u;
            c = (unsigned)cn;
            par ^= 1u;
        }
        // every wave has read its operands of this round (barriers since): the ring slot may be overwritten as far as this
        // workgroup is concerned
        if (tid_k == 0) __hip_atomic_store(RA.wg_round + wg, r + 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (RA.log && r < (unsigned)RA.log_rounds) {           // uniform (mvfit_profile only)
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // this wave's vertex stores have been acknowledged
            __syncthreads();
            if (tid_k == 0) {
                unsigned long long* lg = RA.log + ((size_t)r * gridDim.x + wg) * 2;
                lg[0] = (unsigned long long)ctl[2] | ((unsigned long long)ctl[3] << 32);
                lg[1] = (unsigned long long)wall_clock64();
            }
        }
        // (a round's first chunk goes to buffer 0 whatever the last one used: every request of this round has landed and
        // every wave is behind the closing barrier of its last chunk)
    }
    // whatever ended the loop: nothing waits for this workgroup any more
    if (tid_k == 0) __hip_atomic_store(RA.wg_round + wg, 0xffffffffu, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ---------------------------------------------------------------------------------------------------------
// Resident pass, two tiles per workgroup, with the workgroup split by ROLE (more than 32 problems per optimiser launch: the
// per-GPU shares of BASELINE configs[3] / [4], where the pass has 108 workgroups for 216 tiles).
//
// The kernel above runs a chunk's phases one after the other on all eight waves: contraction (2.4-3.0 k cycles: the matrix
// pipe), barrier, two tiles' blend / apply / stores (3.6 k: LDS gathers), waits (profiles/r5_resident_timeline.log: 8.9 k
// cycles per chunk).  The matrix pipe and the LDS are different units: here they work at the same time.
//   * waves 0-3 (one per SIMD) = CONTRACTION waves: wave w owns tile w & 1, K half w >> 1, all three coordinate planes - three
//     independent 21-MFMA chains interleaved (no dependent-issue bubbles), 168 VGPRs of basis.  While the workers blend chunk
//     k they request chunk k + 1's transforms into the other of two buffers, contract chunk k and write its partials; while
//     the workers apply, they request the coefficient words of chunk k + 1 into the single buffer.
//   * waves 4-7 = WORKERS: the 1024 (vertex pair, problem, tile) items of a chunk, four per thread: blend all four with 24
//     transform rows in flight (one worker wave per SIMD: loads in flight hide the LDS latency, not other waves), then K
//     halves combined, T applied, "+ transl", stores straight from registers.
//   * two bare barriers per chunk: P (blend done | partials published, next contraction done), Y (apply done | the next
//     chunk's operands landed).
// The chains, the blend and the apply are those of the kernel above: the same bits (tests/test_gpu_async.py).
// LDS: transforms 2 x 36 KiB, coefficient words 28 KiB, partials 49.5 KiB, tables: 155.5 KB.
// ---------------------------------------------------------------------------------------------------------
// vmcnt(0) as an instruction the compiler's wait-count pass SEES (an asm statement is opaque to it: it would then take every earlier
// LDS-DMA request for still in flight and put its own vmcnt(0) before the next read of that LDS object - in the middle of the
// requests issued since).  gfx9 encoding: vmcnt = 0, expcnt = 7, lgkmcnt = 15 (untouched)
__device__ __forceinline__ void wait_vm0() {
    __builtin_amdgcn_s_waitcnt(0x0F70);
    asm volatile("" ::: "memory");
}

template <bool HALF>
__global__ __launch_bounds__(VP_NT) __attribute__((amdgpu_waves_per_eu(2, 2))) void lbs_vertex_pass_resident_roles_kernel(DevModel M, ResidentArgs RA) {
    constexpr int TPW = 2;
    __shared__ __attribute__((aligned(16))) f32x4 A_0[32 * A_STRIDE / 4];      // skinning transforms, two chunks
    __shared__ __attribute__((aligned(16))) f32x4 A_1[32 * A_STRIDE / 4];
    __shared__ __attribute__((aligned(16))) f32x4 coef_s[VP_NBLK * 2 * 64];    // [VP_NBLK][hi, lo][64 lanes] A operands of the chunk being contracted
    __shared__ __attribute__((aligned(16))) f32x4 tau_0[32];
    __shared__ __attribute__((aligned(16))) f32x4 tau_1[32];
    __shared__ float part[TPW * 2 * 3 * 32 * 33];                             // [tile][K half][plane][32][33]
    __shared__ f32x4 sw_l[TPW * 32];
    __shared__ i32x4 sj_l[TPW * 32];
    __shared__ float vt_l[4 * 3 * 64];                                        // v_template rows of the contraction waves' chains
    __shared__ unsigned ctl[8];

    const int tid_k = threadIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane(tid_k >> 6);
    const int wg = blockIdx.x;
    const unsigned nch = (unsigned)(RA.n + 31) >> 5;

    // The two roles are two separate loops (the basis registers exist only in the contraction waves' one: in a common loop
    // they would be live at every program point of the workers' code as well).  Both execute the same barriers per round:
    //   S (verdict), Q (first chunk's operands), then per chunk P (blend done / contraction done, partials published) and
    //   Y (apply done / next operands landed).
    if (wave < 4) {
        // ======================================== contraction waves ========================================
#if defined(VPX) && (VPX & 1)
        __builtin_amdgcn_s_setprio(3);
#endif
        const int t_w = wave & 1, kh_w = (wave >> 1) & 1;                      // this wave's tile and K half
        float4 bh[3][VP_BPW], bl[HALF ? 1 : 3][HALF ? 1 : VP_BPW];
        {
            const int lane = tid_k & 63;
            const int tile = min(wg * TPW + t_w, M.ntiles - 1);               // (a tile past the end is never stored)
#pragma unroll
            for (int kc = 0; kc < 3; ++kc) {
                vt_l[(wave * 3 + kc) * 64 + lane] = kh_w == 0 ? M.vt_planes[kc * M.nv_pad + tile * TILE_V + (lane & 31)] * M.bs_scale : 0.f;
                const float4* cb = M.bs_h2 + ((size_t)((tile * 3 + kc) * VP_NBLK + kh_w * VP_BPW) * 2) * 64 + lane;
#pragma unroll
                for (int g = 0; g < VP_BPW; ++g) {
                    bh[kc][g] = nt_load16(&cb[(2 * g) * 64]);
                    if (!HALF) bl[kc][g] = nt_load16(&cb[(2 * g + 1) * 64]);
                }
            }
        }
        __syncthreads();
        // requests (these four waves): transforms 36 x 1 KiB + translations, coefficient words 28 x 1 KiB
        auto request_A = [&](auto Q_, unsigned slot, unsigned c, int lane) {
            constexpr int Q = decltype(Q_)::value;
            const float4* asrc = reinterpret_cast<const float4*>(RA.Amat) + ((size_t)slot * RA.rb + c * 32u) * 72 + lane;
            static_assert(A_STRIDE == 288, "a chunk's transforms are one linear 36 KiB copy");
            // wave w: the nine consecutive KiB from 9 w on; the instruction offset (0 .. 3 KiB) moves BOTH addresses, so four
            // requests share one global address and one M0 - a request is then two instructions, not eight
            const float4* g = asrc + 9 * wave * 64;
            static_for(std::make_integer_sequence<int, 9>{}, [&](auto K_) {
                constexpr int k = decltype(K_)::value;
                if constexpr (Q == 0) __builtin_amdgcn_global_load_lds(g + (k >> 2) * 256, &A_0[(9 * wave + (k & ~3)) * 64], 16, (k & 3) * 1024, /*aux = sc1*/ 16);
                else __builtin_amdgcn_global_load_lds(g + (k >> 2) * 256, &A_1[(9 * wave + (k & ~3)) * 64], 16, (k & 3) * 1024, 16);
            });
            if (wave == 3 && lane < 32) {
                const float4* tsrc = reinterpret_cast<const float4*>(RA.tau) + ((size_t)slot * RA.rb + c * 32u) + lane;
                if constexpr (Q == 0) __builtin_amdgcn_global_load_lds(tsrc, &tau_0[0], 16, 0, 16);
                else __builtin_amdgcn_global_load_lds(tsrc, &tau_1[0], 16, 0, 16);
            }
        };
        auto request_coef = [&](unsigned slot, unsigned c, int lane) {
            const float4* csrc = RA.coefH + ((size_t)slot * ((unsigned)RA.rb >> 5) + c) * (VP_NBLK * 2 * 64) + lane;
            static_assert(VP_NBLK * 2 == 28, "seven KiB per contraction wave");
            const float4* g = csrc + 7 * wave * 64;
            static_for(std::make_integer_sequence<int, 7>{}, [&](auto K_) {
                constexpr int k = decltype(K_)::value;
                __builtin_amdgcn_global_load_lds(g + (k >> 2) * 256, &coef_s[(7 * wave + (k & ~3)) * 64], 16, (k & 3) * 1024, 16);
            });
        };
        // the wave's three chains: small products first, one accumulator per plane.  The A operands of block g + 1 are read
        // into the SAME registers as soon as block g's MFMAs that take them have issued (an MFMA reads its operands at issue):
        // the lo words under six MFMAs, the hi words under the next block's first three - no second operand set (registers)
        // (round 6: a second operand set - block g + 1's words requested before block g's nine MFMAs - measured: the same 3.0 k
        // cycles per 63 MFMAs, i.e. the operand reads are not what holds the stream at 49 cycles per MFMA; 256 VGPRs: not kept)
        auto contract = [&](floatx16 (&acc)[3], int lane) {
#pragma unroll
            for (int kc = 0; kc < 3; ++kc) {
                const float v0 = vt_l[(wave * 3 + kc) * 64 + lane];
#pragma unroll
                for (int q = 0; q < 16; ++q) acc[kc][q] = v0;
            }
            const int cl = (kh_w * VP_BPW * 2) * 64 + lane;
            f32x4 a_h = coef_s[cl], a_l = coef_s[cl + 64];
#pragma unroll
            for (int g = 0; g < VP_BPW; ++g) {
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int kc = 0; kc < 3; ++kc)
                    acc[kc] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(half8, a_l), __builtin_bit_cast(half8, bh[kc][g]), acc[kc], 0, 0, 0);
                __builtin_amdgcn_sched_barrier(0);
                if (g + 1 < VP_BPW) a_l = coef_s[cl + (2 * g + 3) * 64];
                __builtin_amdgcn_sched_barrier(0);
                if (!HALF) {
#pragma unroll
                    for (int kc = 0; kc < 3; ++kc)
                        acc[kc] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(half8, a_h), __builtin_bit_cast(half8, bl[HALF ? 0 : kc][HALF ? 0 : g]), acc[kc], 0, 0, 0);
                }
#pragma unroll
                for (int kc = 0; kc < 3; ++kc)
                    acc[kc] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(half8, a_h), __builtin_bit_cast(half8, bh[kc][g]), acc[kc], 0, 0, 0);
                __builtin_amdgcn_sched_barrier(0);
                if (g + 1 < VP_BPW) a_h = coef_s[cl + (2 * g + 2) * 64];
            }
        };
        auto put_partials = [&](const floatx16 (&acc)[3], int lane) {
#pragma unroll
            for (int kc = 0; kc < 3; ++kc) {
                const int p0 = (((t_w * 2 + kh_w) * 3 + kc) * 32 + 4 * (lane >> 5)) * 33 + (lane & 31);
#pragma unroll
                for (int q = 0; q < 16; ++q) part[p0 + ((q & 3) + 8 * (q >> 2)) * 33] = acc[kc][q];
            }
        };
        for (unsigned r = 0; r < RA.max_rounds; ++r) {
            const unsigned slot = r % (unsigned)RA.nslots;
            __syncthreads();                                                  // (S) wave 7's verdict
            const unsigned verdict = ctl[0];
            unsigned mask = ctl[1];
            if (verdict == VR_LOST) { __syncthreads(); continue; }            // (S') round skipped (see resident_poll)
            if (verdict != VR_GO) break;                                      // uniform
            int lane = tid_k & 63;
            asm volatile("" : "+v"(lane));                                    // (opaque copy: no address hoisting out of the round loop)
            unsigned c = (unsigned)__builtin_ctz(mask);
            mask &= mask - 1u;
            int cn = mask ? __builtin_ctz(mask) : -1;
            // ---- the round's first live chunk: its operands ----
            request_A(std::integral_constant<int, 0>{}, slot, c, lane);
            request_coef(slot, c, lane);
            wait_vm0();
            wg_barrier_lds();                                                 // (Q)
            unsigned par = 0u;                                                // transform buffer of the chunk the workers blend
            // one chunk (transform buffer P holds its transforms, the coefficient buffer its words): the next chunk's transforms
            // requested into the other buffer, then the contraction and the partials, while the workers blend; then, while they
            // apply and store, the next chunk's coefficient words into the single buffer (every contraction wave is past P:
            // the words have been read).  No work is done ahead of the workers: a round has no pipeline to fill.
            auto chunk = [&](auto P_, int cn) {
                constexpr int P = decltype(P_)::value;
#ifdef MVFIT_TIMING
                const long long t_ch = clock64();              // timeline of a middle chunk (steady state), tests/vp_resident_timeline.py
#define VPQ_T(k_) do { if (P == 1 && cn >= 0) VP_T(k_, t_ch); } while (0)
#else
#define VPQ_T(k_) do { } while (0)
#endif
                if (cn >= 0) request_A(std::integral_constant<int, 1 - P>{}, slot, (unsigned)cn, lane);
                VPQ_T(0);
                floatx16 acc[3];
                contract(acc, lane);
                VPQ_T(1);
                put_partials(acc, lane);
                VPQ_T(2);
                wg_barrier_lds();                                             // (P) partials published; the workers have blended
                VPQ_T(3);
                if (cn >= 0) request_coef(slot, (unsigned)cn, lane);
                VPQ_T(4);
                wait_vm0();                                                   // this wave's requests have landed
                VPQ_T(5);
                wg_barrier_lds();                                             // (Y) the workers have applied
                VPQ_T(6);
#ifdef MVFIT_TIMING
                if (P == 1 && cn >= 0 && blockIdx.x == 5 && (tid_k & 255) == 0) g_vp[7 + (tid_k >> 8) * 8] += 1;
#endif
            };
            for (;;) {
                if (par == 0u) chunk(std::integral_constant<int, 0>{}, cn);
                else chunk(std::integral_constant<int, 1>{}, cn);
                if (cn < 0) break;
                mask &= mask - 1u;
                cn = mask ? __builtin_ctz(mask) : -1;
                par ^= 1u;
            }
            if (RA.log && r < (unsigned)RA.log_rounds) __syncthreads();       // (the workers' log barrier)
        }
        return;
    }

    // ================================================ workers ================================================
#if defined(VPX) && (VPX & 4)
    const bool store_nt = false;
#else
    const bool store_nt = VP_NT_LOADS && !(RA.flags & 2u);
#endif
    const float inv_scale = 1.0f / M.bs_scale;
    {
        const int wt = tid_k - 256;
        if (wt < 64) sw_l[wt] = __builtin_bit_cast(f32x4, M.wsp_w[(size_t)min(wg * TPW + (wt >> 5), M.ntiles - 1) * TILE_V + (wt & 31)]);
        else if (wt < 128) sj_l[wt - 64] = __builtin_bit_cast(i32x4, M.wsp_j[(size_t)min(wg * TPW + ((wt - 64) >> 5), M.ntiles - 1) * TILE_V + (wt & 31)]);
    }
    __syncthreads();
    // Round 6: the two vertices of a thread's pair mostly hang on the SAME four joints (neighbours in the mesh: 93 % of the pairs
    // of the synthetic body, most of SMPL's) - then the second vertex blends the transform rows the first one fetched (other
    // weights, the same rows: the same products in the same order, bit-identical) and the pair costs 24 LDS gathers instead of
    // 48.  The gathers were the blend phase's bound: 4 worker waves x 96 ds_read_b128 = 3.1 k cycles of LDS port per chunk
    // (profiles/r5_pmc_lds_resident.json: 2.9 k measured) against 1.8 k cycles of FMA issue.
    bool pair_same[TPW];
    {
        const int vp2 = (tid_k - 256) & 15;
#pragma unroll
        for (int t = 0; t < TPW; ++t) {
            const i32x4 a = sj_l[t * 32 + 2 * vp2], b = sj_l[t * 32 + 2 * vp2 + 1];
            pair_same[t] = a.x == b.x && a.y == b.y && a.z == b.z && a.w == b.w;
        }
    }
    unsigned lost_total = 0u;                                   // (polling wave) operand sets this workgroup lost so far
    for (unsigned r = 0; r < RA.max_rounds; ++r) {
        const unsigned slot = r % (unsigned)RA.nslots;
        // ---- wave 7: wait for the operands of closure round r (every problem: published, or finished before r) ----
        if (wave == 7) resident_poll(RA, r, slot, nch, tid_k & 63, wg, ctl, lost_total);
        __syncthreads();                                                      // (S)
        const unsigned verdict = ctl[0];
        unsigned mask = ctl[1];
        if (verdict == VR_LOST) {                                             // uniform: skip the round (see resident_poll)
            __syncthreads();                                                  // (S') every wave has read ctl
            if (tid_k == 256) __hip_atomic_store(RA.wg_round + wg, r + 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            continue;
        }
        if (verdict != VR_GO) break;                                          // uniform
        float* vout = (RA.capture_verts && (int)r == RA.capture_round) ? RA.capture_verts : RA.verts;
        unsigned c = (unsigned)__builtin_ctz(mask);
        mask &= mask - 1u;
#ifdef MVFIT_TIMING
        const long long t_round = clock64();                                  // whole rounds (tests/vp_resident_timeline.py): S -> Q -> end
        const bool t_full = __popc(ctl[1]) == 4;
#endif
        wg_barrier_lds();                                                     // (Q)
#ifdef MVFIT_TIMING
        if (t_full) VP_T(4, t_round);
#endif
        unsigned par = 0u;                                                    // transform buffer of the chunk being blended
        for (;;) {
            const int cn = mask ? __builtin_ctz(mask) : -1;
            int tid = tid_k;
            asm volatile("" : "+v"(tid));                                     // (opaque copy: no address hoisting out of the round loop)
#ifdef MVFIT_TIMING
            const long long t_wk = clock64();
            const bool t_mid = cn >= 0 && c != (unsigned)__builtin_ctz(ctl[1]);      // a middle chunk of the round
#define VPW_T(k_) do { if (t_mid) VP_T(k_, t_wk); } while (0)
#else
#define VPW_T(k_) do { } while (0)
#endif
            // ---- four items per thread = (vertex pair vp2) x (problems q, q + 16) x (tiles 0, 1): blend all four (the
            //      transforms are then free for the next chunk's request) ----
            const int wt = tid - 256, vp2 = wt & 15, q = wt >> 4;
            // (the blend as packed FMAs - v_pk_fma_f32 on (x, y) / (z, w) halves, 216 instead of 413 FMA instructions - measured
            // SLOWER in round 6: 15.4 instead of 13.8 us per round; a packed fp32 FMA does not issue faster than two scalar ones
            // here and the weight pairs cost 50 moves)
            float tr[4][2][3][4];                                             // [item = 2 t + e][vertex][row][4]
#pragma unroll
            for (int t = 0; t < TPW; ++t) {
                f32x4 rows[2][4][3];
#pragma unroll
                for (int i = 0; i < 2; ++i) {
                    const f32x4 spw = sw_l[t * 32 + 2 * vp2 + i];
                    const i32x4 spj = sj_l[t * 32 + 2 * vp2 + i];
                    const float wq[4] = {spw.x, spw.y, spw.z, spw.w};
                    const int jq[4] = {spj.x, spj.y, spj.z, spj.w};
                    // one vertex of the tile for BOTH of the thread's problems: 24 transform rows requested before the first
                    // product (one worker wave per SIMD: the latency of the LDS gathers is hidden by loads in flight, not by
                    // other waves); ascending joint order per item: the non-zero products of the dense blend in the same order.
                    // The pair's second vertex keeps the first one's rows when it hangs on the same joints (pair_same)
                    if (i == 0 || !pair_same[t]) {
#pragma unroll
                        for (int e = 0; e < 2; ++e)
#pragma unroll
                            for (int u = 0; u < 4; ++u)
#pragma unroll
                                for (int k = 0; k < 3; ++k) {
                                    const int at = (q + 16 * e) * (A_STRIDE / 4) + jq[u] * 3 + k;
                                    rows[e][u][k] = par ? A_1[at] : A_0[at];      // (uniform)
                                }
                    }
#pragma unroll
                    for (int e = 0; e < 2; ++e) {
#pragma unroll
                        for (int k = 0; k < 3; ++k)
#pragma unroll
                            for (int z = 0; z < 4; ++z) tr[2 * t + e][i][k][z] = 0.f;
#pragma unroll
                        for (int u = 0; u < 4; ++u)
#pragma unroll
                            for (int k = 0; k < 3; ++k) {
                                const f32x4 a = rows[e][u][k];
                                tr[2 * t + e][i][k][0] = fmaf(wq[u], a.x, tr[2 * t + e][i][k][0]);
                                tr[2 * t + e][i][k][1] = fmaf(wq[u], a.y, tr[2 * t + e][i][k][1]);
                                tr[2 * t + e][i][k][2] = fmaf(wq[u], a.z, tr[2 * t + e][i][k][2]);
                                tr[2 * t + e][i][k][3] = fmaf(wq[u], a.w, tr[2 * t + e][i][k][3]);
                            }
                        // (the products are pinned HERE: instruction selection otherwise emits the row loads of all four items
                        // first and the FMAs behind them - 384 registers of rows in flight)
#pragma unroll
                        for (int k = 0; k < 3; ++k)
                            asm volatile("" : "+v"(tr[2 * t + e][i][k][0]), "+v"(tr[2 * t + e][i][k][1]), "+v"(tr[2 * t + e][i][k][2]),
                                              "+v"(tr[2 * t + e][i][k][3]));
                    }
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
            const f32x4 tq0 = par ? tau_1[q] : tau_0[q], tq1 = par ? tau_1[q + 16] : tau_0[q + 16];
            VPW_T(1);
            wg_barrier_lds();                                                 // (P)
            VPW_T(2);
            // ---- K halves combined (fixed order), scale undone, T applied, "+ transl", stores straight from registers ----
            // (24 contiguous bytes per item - vertices 2 vp2, 2 vp2 + 1 -, 8-byte aligned: even vertex count, checked by the host)
            // (b_me: the problem the ring row held in this round - the translation word's spare lane, see the kernel above;
            // rows whose problem does not evaluate this round are not stored)
            const unsigned live_rows = ctl[4 + c];
            auto store_item = [&](const float (&o)[6], int t, int e, int tq, int b_me) {
                const int vbase = (wg * TPW + t) * TILE_V, vq = tq & 15;
                const int nv_ok = ((live_rows >> ((tq >> 4) + 16 * e)) & 1u) ? min(TILE_V, M.nv - vbase) - 2 * vq : 0;
                float* dst = vout + ((size_t)b_me * M.nv + vbase + 2 * vq) * 3;
#if defined(VPX) && (VPX & 2)
                if (o[0] == 1.2345e-30f) dst[0] = o[1] + o[2] + o[3] + o[4] + o[5];      // (experiment: no stores)
#else
                if (nv_ok >= 2) {
                    const f32x2 q0 = {o[0], o[1]}, q1 = {o[2], o[3]}, q2 = {o[4], o[5]};
                    if (store_nt) {
                        __builtin_nontemporal_store(q0, reinterpret_cast<f32x2*>(dst));
                        __builtin_nontemporal_store(q1, reinterpret_cast<f32x2*>(dst + 2));
                        __builtin_nontemporal_store(q2, reinterpret_cast<f32x2*>(dst + 4));
                    } else {
                        *reinterpret_cast<f32x2*>(dst) = q0; *reinterpret_cast<f32x2*>(dst + 2) = q1; *reinterpret_cast<f32x2*>(dst + 4) = q2;
                    }
                } else if (nv_ok == 1) {
                    dst[0] = o[0]; dst[1] = o[1]; dst[2] = o[2];
                }
#endif
            };
            // (Round 6, measured on the stores - a chunk's 24.6 KB cost the workers ~1 k of the apply's 2.2 k cycles: 14.0 -> 11.9 us
            // per round WITHOUT them.  16 + 8 bytes per item, lane-pair 16-byte words by DPP, whole 1 KiB lines per instruction
            // staged through the dead transform buffer (3.2 k), the last tile's stores behind (Y) (the wave blocks there instead),
            // plain instead of non-temporal: none faster than three 8-byte stores per item - the CU's write path takes ~10 bytes
            // per clock whatever the shape; profiles/r6_progress.md)
#pragma unroll
            for (int t = 0; t < TPW; ++t) {
                const int tile = wg * TPW + t;
                if (tile >= M.ntiles) break;                                  // uniform
                const int pt = t * (2 * 3 * 32 * 33);
#pragma unroll
                for (int e = 0; e < 2; ++e) {
                    const int bb = q + 16 * e;
                    const float tau3[3] = {e ? tq1.x : tq0.x, e ? tq1.y : tq0.y, e ? tq1.z : tq0.z};
                    float o[6];
                    // (the pair's two vertices are neighbours in a row of partials and are read side by side; the compiler keeps
                    // single ds_read_b32 all the same - rows start at odd dword offsets - and the round measures the same)
                    float vp[2][3];
#pragma unroll
                    for (int k = 0; k < 3; ++k) {
                        const int p0 = pt + ((0 * 3 + k) * 32 + bb) * 33 + 2 * vp2, p1 = pt + ((1 * 3 + k) * 32 + bb) * 33 + 2 * vp2;
                        const float a0 = part[p0], a1 = part[p0 + 1], b0 = part[p1], b1 = part[p1 + 1];
                        vp[0][k] = (a0 + b0) * inv_scale;
                        vp[1][k] = (a1 + b1) * inv_scale;
                    }
#pragma unroll
                    for (int i = 0; i < 2; ++i)
#pragma unroll
                        for (int k = 0; k < 3; ++k)
                            o[3 * i + k] = fmaf(tr[2 * t + e][i][k][0], vp[i][0], fmaf(tr[2 * t + e][i][k][1], vp[i][1],
                                                fmaf(tr[2 * t + e][i][k][2], vp[i][2], tr[2 * t + e][i][k][3]))) + tau3[k];
                    const float row_prob = e ? tq1.w : tq0.w;             // (a float rvalue first: see the kernel above)
                    store_item(o, t, e, wt, __builtin_bit_cast(int, row_prob));
                }
            }
            VPW_T(3);
            wg_barrier_lds();                                                 // (Y)
            VPW_T(6);
#ifdef MVFIT_TIMING
            if (t_mid && blockIdx.x == 5 && (tid_k & 255) == 0) g_vp[7 + (tid_k >> 8) * 8] += 1;
#endif
            if (cn < 0) break;
            mask &= mask - 1u;
            c = (unsigned)cn;
            par ^= 1u;
        }
#ifdef MVFIT_TIMING
        if (t_full) { VP_T(5, t_round); if (blockIdx.x == 5 && tid_k == 256) g_vp[8] += 1; }
#endif
        // every operand of this round has been read (the contraction waves waited for their requests before the last (Y))
        if (tid_k == 256) __hip_atomic_store(RA.wg_round + wg, r + 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (RA.log && r < (unsigned)RA.log_rounds) {                          // uniform (mvfit_profile only)
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                  // this wave's vertex stores have been acknowledged
            __syncthreads();
            if (tid_k == 256) {
                unsigned long long* lg = RA.log + ((size_t)r * gridDim.x + wg) * 2;
                lg[0] = (unsigned long long)ctl[2] | ((unsigned long long)ctl[3] << 32);
                lg[1] = (unsigned long long)wall_clock64();
            }
        }
    }
    // whatever ended the loop: nothing waits for this workgroup any more
    if (tid_k == 256) __hip_atomic_store(RA.wg_round + wg, 0xffffffffu, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// form 1: one tile per workgroup (lbs_vertex_pass_resident_kernel<1>); form 3 (and the former form 2, which it replaced: the
// one-tile kernel's code with two tiles was 30 % slower and is no longer instantiated - round 6): two tiles per workgroup,
// contraction / worker roles.  grid = ceil(ntiles / tiles) workgroups, all of which must be resident
hipError_t launch_vertex_pass_resident(const DevModel& M, const ResidentArgs& RA, int tpw, hipStream_t stream) {
    if (tpw >= 2) {
        const dim3 grid((M.ntiles + 1) / 2);
        hipLaunchKernelGGL(M.half_basis ? lbs_vertex_pass_resident_roles_kernel<true> : lbs_vertex_pass_resident_roles_kernel<false>,
                           grid, dim3(VP_NT), 0, stream, M, RA);
        return hipGetLastError();
    }
    const dim3 grid(M.ntiles);
    auto kern = M.half_basis ? lbs_vertex_pass_resident_kernel<1, true> : lbs_vertex_pass_resident_kernel<1, false>;
    hipLaunchKernelGGL(kern, grid, dim3(VP_NT), 0, stream, M, RA);       // (static LDS)
    return hipGetLastError();
}

size_t vertex_pass_pipe_lds_bytes() {
    return sizeof(float) * (size_t)(2 * 32 * A_STRIDE + 3 * 32 * 33 + 2 * 32 * 4) + 16 * (size_t)(2 * VP_NBLK * 2 * 64 + 32 + 32) + 4 * (32 + 4 + 64);
}

size_t vertex_pass_split_lds_bytes() {
    return sizeof(float) * (size_t)(32 * A_STRIDE + 4 * NJ * 32 + 32 * 4 + 2 * 3 * 32 * 33 + 2 * 32 * 96);
}
size_t vertex_pass_split_loop_lds_bytes() {
    return sizeof(float) * (size_t)(32 * A_STRIDE + 4 * NJ * 32 + 2 * 32 * 4 + 2 * 3 * 32 * 33 + 2 * 32 * 96 + VP_NBLK * 2 * 64 * 4 + 4);
}

size_t vertex_pass_lds_bytes() {
    return sizeof(float) * (size_t)(KROWS * 32 + 32 * A_STRIDE + 4 * NJ * 32 + 32 * 4 +
                                    VP_KSPLIT * 3 * 32 * 33 + 2 * 32 * 96);
}

// ev_start / ev_stop (both or neither): the runtime stamps them with the dispatch's own begin / end (hipExtLaunchKernelGGL)
// - the kernel's duration without the few microseconds a pair of hipEventRecord markers around a launch would add.
template <typename K>
static void vp_launch(K kernel, dim3 grid, size_t lds, hipStream_t stream, hipEvent_t ev_start, hipEvent_t ev_stop,
                      const DevModel& M, const DevPose& P, int B, float* verts) {
    if (ev_start) hipExtLaunchKernelGGL(kernel, grid, dim3(VP_NT), lds, stream, ev_start, ev_stop, 0, M, P, B, verts);
    else hipLaunchKernelGGL(kernel, grid, dim3(VP_NT), lds, stream, M, P, B, verts);
}

// Which kernel serves chunks [P.chunk0, ceil(B / 32)) is plan_pass_launch's decision (fit_plan.cpp; the table: DESIGN.md §4.4):
// the exact-fp32 chain without the split-fp16 basis; with it one workgroup per (tile, chunk) for a single chunk or
// pass_kernel 1, else one workgroup per vertex tile that walks ALL chunks with the tile's basis held in registers - the
// two-role pipeline for <= 4 weights per vertex and an even vertex count, the lock-step loop for dense skinning rows.
// pass_kernel 2 is 0: the lock-step loop's <= 4-weights instantiation, which it used to select, is gone (round 6), and an odd
// vertex count with <= 4 weights takes one workgroup per (tile, chunk).
hipError_t launch_vertex_pass(const DevModel& M, const DevPose& P, int B, float* verts, int pass_kernel,
                              hipStream_t stream, hipEvent_t ev_start, hipEvent_t ev_stop) {
    const PassLaunch L = plan_pass_launch(M.bs_h2 != nullptr, M.wsp_w != nullptr, (M.nv & 1) == 0, (B + 31) / 32 - P.chunk0, pass_kernel);
    const dim3 grid(M.ntiles, L.grid_y);
    switch (L.kernel) {
    case PASS_EXACT:
        if (L.sparse) vp_launch(lbs_vertex_pass_kernel<true>, grid, vertex_pass_lds_bytes(), stream, ev_start, ev_stop, M, P, B, verts);
        else vp_launch(lbs_vertex_pass_kernel<false>, grid, vertex_pass_lds_bytes(), stream, ev_start, ev_stop, M, P, B, verts);
        break;
    case PASS_SPLIT:
        if (L.sparse) vp_launch(lbs_vertex_pass_split_kernel<true>, grid, vertex_pass_split_lds_bytes(), stream, ev_start, ev_stop, M, P, B, verts);
        else vp_launch(lbs_vertex_pass_split_kernel<false>, grid, vertex_pass_split_lds_bytes(), stream, ev_start, ev_stop, M, P, B, verts);
        break;
    case PASS_SPLIT_LOOP:
        vp_launch(lbs_vertex_pass_split_loop_kernel<false>, grid, vertex_pass_split_loop_lds_bytes(), stream, ev_start, ev_stop, M, P, B, verts);
        break;
    case PASS_PIPE:
        vp_launch(lbs_vertex_pass_pipe_kernel, grid, vertex_pass_pipe_lds_bytes(), stream, ev_start, ev_stop, M, P, B, verts);
        break;
    default:
        return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

hipError_t vertex_pass_configure() {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(lbs_vertex_pass_kernel<false>),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)vertex_pass_lds_bytes());
    if (e != hipSuccess) return e;
    e = hipFuncSetAttribute(reinterpret_cast<const void*>(lbs_vertex_pass_kernel<true>),
                            hipFuncAttributeMaxDynamicSharedMemorySize, (int)vertex_pass_lds_bytes());
    if (e != hipSuccess) return e;
    e = hipFuncSetAttribute(reinterpret_cast<const void*>(lbs_vertex_pass_split_kernel<false>),
                            hipFuncAttributeMaxDynamicSharedMemorySize, (int)vertex_pass_split_lds_bytes());
    if (e != hipSuccess) return e;
    e = hipFuncSetAttribute(reinterpret_cast<const void*>(lbs_vertex_pass_split_kernel<true>),
                            hipFuncAttributeMaxDynamicSharedMemorySize, (int)vertex_pass_split_lds_bytes());
    if (e != hipSuccess) return e;
    e = hipFuncSetAttribute(reinterpret_cast<const void*>(lbs_vertex_pass_split_loop_kernel<false>),
                            hipFuncAttributeMaxDynamicSharedMemorySize, (int)vertex_pass_split_loop_lds_bytes());
    if (e != hipSuccess) return e;
    return hipFuncSetAttribute(reinterpret_cast<const void*>(lbs_vertex_pass_pipe_kernel),
                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)vertex_pass_pipe_lds_bytes());
}

}  // namespace mvfit

#ifdef MVFIT_TIMING
extern "C" __attribute__((visibility("default"))) int mvfit_debug_vp(long long* out16) {
    (void)hipDeviceSynchronize();
    return (int)hipMemcpyFromSymbol(out16, HIP_SYMBOL(mvfit::g_vp), sizeof(long long) * 16);
}
#endif
