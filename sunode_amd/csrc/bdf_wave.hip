/*
 * bdf_wave.hip -- one wavefront per instance, LDS-resident dense LU (64 < max(n, p) <= 128; gfx950).
 *
 * The mapping for mid-size systems whose batches are small (BASELINE config 5: 100 states, 1024
 * instances per GPU): a whole wavefront integrates ONE instance.
 *   - component c of every vector lives in lane c % 64, slot c / 64 (RS = ceil(n/64) slots), so the
 *     Nordsieck array, weights and corrections are a few dozen VGPRs and every vector update is
 *     pure register arithmetic;
 *   - WRMS norms are xor-butterflies over the wave per slot followed by a pairwise sum of the slot
 *     totals: exactly the balanced tree of the CPU oracle over next_pow2(n) leaves;
 *   - the Newton matrix I - gamma*J lives in LDS, column-major (n^2 doubles: 80 000 B at n = 100,
 *     two workgroups per CU).  The LU with partial pivoting is row-distributed (lane owns rows):
 *     pivot search = wave arg-max, pivot row / pivot entries are LDS broadcast reads, elimination
 *     is n^2/2 conflict-free ds_read/FMA/ds_write triples per lane slot instead of n^3/3 serial
 *     flops; the triangular solves broadcast one entry per step with v_readlane;
 *   - the saved Jacobian and the callback output vector are in an HBM workspace (per instance
 *     contiguous, coalesced);
 *   - the sympy-generated callbacks are straight-line scalar code without exploitable structure:
 *     the wave stages the state in LDS (broadcast reads), every lane evaluates the whole callback
 *     (chunked noinline functions, shared rate constants through scalar loads) and the results go
 *     to LDS (Jacobian) or the workspace vector -- redundant but divergence-free work.
 * Control scalars are recomputed redundantly by all lanes from identical inputs (uniform control
 * flow without votes).
 *
 * Same algorithm, operation order and rounding as the other builds / the CPU oracle (restated
 * CVODES 5.x; reference call sites /root/reference/sunode/solver.py:467-527, 682-784).
 * Kernel entry points and argument blocks are those of bdf_kernels.hip; sa_meta = {n, p, r, ABI,
 * 64 * SA_WAVES lanes per instance (= workgroup size), workspace doubles per instance}.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>

/* the build passes the sizes (parsed from the generated header) because the LDS arrays the
   generated code reads must be declared before that header is included */
#if !defined(SA_BUILD_NS) || !defined(SA_BUILD_NQ)
#error "SA_BUILD_NS / SA_BUILD_NQ must be defined"
#endif
#define W_NS SA_BUILD_NS
#define W_NQ SA_BUILD_NQ

/* Lanes per instance: 64 (a whole wavefront, the default) or a smaller power of two >= max(n, p)
   (SA_GROUP = 8..32: 64/G instances share a wavefront, every instance has its own slice of the LDS
   arrays; the mapping for systems of 6..64 states). */
#ifndef SA_GROUP
#define SA_GROUP 64
#endif
#if SA_GROUP < 64
#undef SA_WAVES
#define SA_WAVES 1                   /* worker wavefronts need the whole-wavefront mapping */
#define G SA_GROUP
#else
#define G 64
#endif
#define KPW (64 / G)
#define W_NQD (W_NQ > 0 ? W_NQ : 1)
#define W_PIV ((W_NS + 15) / 16 * 16)
/* LEAN lane groups (G < 64 and at most 64 matrix doubles per lane, i.e. n <= 16 with four lanes, n <= 21 with eight):
   the LU factors stay in REGISTERS between factorisation and solves (static DPP broadcasts, no LDS matrix at all --
   16 instances x 2 KB would not fit next to the rest), the Jacobian callback writes straight to the saved copy in the
   workspace, and the cold per-instance state (interpolation table) lives in LDS instead of registers. */
#define W_RS_PRE ((W_NS + G - 1) / G)
#if SA_GROUP <= 8 && (W_NS * W_RS_PRE) <= 64
#define SA_LEAN 1
#else
#define SA_LEAN 0
#endif
/* a group's slice of the staging vectors starts at an ODD multiple-free stride (doubles): with a power-of-two n
   the 64/G groups of a wavefront hit the same few banks when they read "their" element i (16 x 16 states: 8-way
   conflict on every callback input), with an odd stride every group has its own bank pair */
#define W_NSP (KPW > 1 ? (W_NS | 1) : W_NS)
#define W_NQP (KPW > 1 ? (W_NQD | 1) : W_NQD)
__shared__ double s_y[KPW * W_NSP];                 /* callback input: state (backward: interpolated forward state) */
#if SA_LEAN && (KPW * W_NSP >= W_NS * W_NS)
#define s_A s_y                                     /* scratch of the pivoting fall-back: ONE matrix, used a group at a time,
                                                       between callbacks (every callback stages its inputs afresh) */
#elif SA_LEAN
__shared__ double s_A[W_NS * W_NS];
#else
__shared__ double s_A[KPW * W_NS * W_NS];           /* Newton matrix / its LU, column-major, per instance */
#endif
__shared__ double s_lam[KPW * W_NSP];               /* callback input: adjoint state; scratch for the LU solves */
__shared__ double s_ps[KPW * W_NQP];                /* differentiated parameters of the instance */
__shared__ uint8_t s_piv[KPW * W_PIV];              /* pivot rows (n <= 128 fits a byte) */
#define W_NOUT (W_NS > W_NQD ? W_NS : W_NQD)
#define W_NOUTP (KPW > 1 ? (W_NOUT | 1) : W_NOUT)
__shared__ double s_out[KPW * W_NOUTP];             /* output vector of the vector-valued callbacks */
/* (the same two parking schemes for wavefront 0 of the workgroup-per-instance build were measured in round 4 -- 100 -> 42
   spill slots, not faster: profiles/r04_network100_lu.txt -- and removed again) */
#define SA_COLD_PARK SA_LEAN
#if SA_LEAN && !defined(SA_HERMITE)
/* the divided-difference record of the current interpolation index, copied from the arena when the index moves
   (20 + 6 n/G registers per lane otherwise).  Stride: even (16-byte rows) and not a multiple of 16 doubles. */
#define SA_TAB_LDS 1
#define W_TREC (8 + 6 * W_NS)
#define W_TRECP (W_TREC + 2)
__shared__ double s_tab[KPW * W_TRECP];
#else
#define SA_TAB_LDS 0
#endif
#if SA_COLD_PARK
/* COLD per-lane state, parked in LDS across the Newton pass of a step attempt (callbacks, factorisation, solves): the
   Nordsieck columns 2..5, the saved correction and the whole quadrature history are only touched by predict / rescale
   / complete / order changes.  Lane-private slots [slot][lane]: no synchronisation, conflict-free. */
#define W_RQ_PRE (W_NQ > 0 ? (W_NQ + G - 1) / G : 1)
#define W_NCOLD (5 * W_RS_PRE + 7 * W_RQ_PRE)
__shared__ double s_cold[W_NCOLD * 64];
/* ... and the group-uniform coefficient vectors the Newton pass does not read: l[0..5], tau[1..5], tq[1], tq[3], tq[5]
   (lane 0 of the group writes, every lane reads them back) */
#define W_NCTL 14
__shared__ double s_ctl[KPW * W_NCTL];
#ifdef SA_SENS
/* The forward-sensitivity builds keep these in registers (parking them there was never measured to pay).  Round 3
   recorded that with l[] parked the 4-lane SEIR build stopped being bit-equal to the oracle -- and that merely reading
   m.l after the Newton pass changed the result.  Round 4 (profiles/r04_sens_anomaly.txt, tools/repro_vgpr_liverange.sh):
   the vectors ARE uniform across the lanes of a group (-DSA_CTL_CHECK), no LDS ordering is involved (a hard barrier
   around the parked values changes nothing), and the wrong results follow one compiler pass: they need
   -disable-machine-licm (which the sensitivity builds then inherited from the adjoint flag set), survive eight other
   code-generation variations and disappear with -mllvm -amdgpu-opt-vgpr-liverange=0, i.e. without SIOptimizeVGPRLiveRange,
   the pass that declares registers dead in the side of a divergent branch a lane does not take.  The failing
   combination is not shipped; SA_VGPR_LIVERANGE_OPT=0 builds every register-resident kernel without the pass
   (_native.py SAFETY_CODEGEN_FLAGS: the conservative build, 10 ... 27 % slower). */
#ifndef SA_SENS_CTL_PARK            /* (experiments) */
#define SA_NO_CTL_PARK 1
#endif
#endif
#endif
/* Workgroup barrier as ONE inline instruction sequence.  In this build pipeline (clang -O0 -> always-inline -> -O3)
   HIP's __syncthreads() stays a real function call: every call site spilled the caller's live VGPRs to scratch and
   reloaded them (140 scratch instructions around the single barrier of the LU's elimination loop -- 14 000 scratch
   accesses per factorisation, the reason a 100 x 100 LU took 190 us). */
#define sa_barrier() do { __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup"); __builtin_amdgcn_s_barrier(); \
                          __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup"); } while (0)
/* index of the calling lane's instance within its wavefront */
static __device__ __forceinline__ int sa_grp()
{
    if (KPW == 1) return 0;
    return (int)(__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u))) / G;
}

/* Worker wavefronts: the workgroup of an instance has SA_WAVES wavefronts.  Wavefront 0 runs the
   integrator; the others sleep on the workgroup barrier and wake up to evaluate their share of the
   chunks of a generated callback (the callbacks dominate the run time and are embarrassingly
   parallel over their output statements). */
#ifndef SA_WAVES
#define SA_WAVES 4
#endif
static_assert(G == 64 || SA_WAVES == 1, "worker wavefronts need 64 lanes per instance");
__shared__ int s_cmd, s_nwaves, s_flag;
__shared__ double s_targ;
__shared__ int s_rc[SA_WAVES];      /* (only s_nwaves is referenced by the single-wavefront builds: the rest costs them no LDS) */
enum { CMD_EXIT = 0, CMD_RHS = 1, CMD_QUAD = 2, CMD_JAC = 3, CMD_GETRF = 4 };
static __device__ __forceinline__ int sa_wave_index() { return __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)); }
/* (s_nwaves is SA_WAVES in the integrator kernels and 1 in sa_k_eval: spelled out, both remainders are compile-time
   -- a remainder by the run-time value costs ~25 instructions, several times per callback and wavefront) */
#define SA_MOD_NWAVES(c) (s_nwaves == SA_WAVES ? (c) % SA_WAVES : (s_nwaves == 1 ? 0 : (c) % s_nwaves))
#define SA_CHUNK_CALL(c, call) do { if (SA_MOD_NWAVES(c) == sa_wave_index()) bad |= call; } while (0)

#define SA_FN static __device__ __attribute__((noinline))
#define SA_TEMPLATE template <class SinkT>
#define SA_OUT_T SinkT
#define SA_STORE(slot, value) out.template put<(slot)>(value)
#define SA_Y(i) sa_yv[i]
#define SA_LAM(i) sa_lv[i]
#define SA_PS(j) sa_pv[j]
#define SA_LDS_VIEWS const double *sa_yv = s_y + sa_grp() * W_NSP; const double *sa_lv = s_lam + sa_grp() * W_NSP; \
    const double *sa_pv = s_ps + sa_grp() * W_NQP; (void)sa_yv; (void)sa_lv; (void)sa_pv;
typedef __attribute__((address_space(1))) double gdouble;      /* explicit global pointer: cannot alias LDS */
#define SA_CONST_AS __attribute__((address_space(4)))
/* remaining parameters: broadcast global loads (all lanes read the same address; the vector memory
   pipe is otherwise idle during a callback and keeps dozens of loads in flight) */
#define SA_PR(j) prg[j]
/* A chunk function touches the parameter ranges it is about to read with ONE load per 8 KB (every lane a
   different 128-byte line); the values are parked in sa_pf[] and only consumed by the epilogue, so nothing
   waits for them -- but the statements' own broadcast loads then hit the L1 instead of paying the L2 latency
   at the head of every statement. */
static __device__ __forceinline__ double sa_touch(const gdouble *p, int n)
{
    const int k = (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u)) * 16;
    return p[k < n ? k : 0];
}
#define SA_PROLOGUE SA_LDS_VIEWS const gdouble *prg = (const gdouble *)pr; \
    double sa_pf[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0}; (void)sa_pf;
#define SA_PREFETCH_PR(k, lo, hi) sa_pf[k] = sa_touch(prg + (lo), (hi) - (lo) + 1)
#define SA_EPILOGUE asm volatile("" :: "v"(sa_pf[0]), "v"(sa_pf[1]), "v"(sa_pf[2]), "v"(sa_pf[3]), \
                                 "v"(sa_pf[4]), "v"(sa_pf[5]), "v"(sa_pf[6]), "v"(sa_pf[7]));
/* Small systems (config 4: n = 16): NO per-statement barriers.  With them every LDS / parameter load of a statement
   is waited for on the spot -- the SEIR adjoint right-hand side was 94 dependent memory round trips (32 of them
   global loads of the contact matrix), 11 k cycles per call; without them the scheduler batches the loads (8 global
   loads, one wait) and the whole SEIR solve is 21 % faster.  The barriers are for the thousands of statements of the
   n = 100 callbacks (below). */
#if W_NS > 32
/* keep the instruction scheduler from hoisting the loads of later statements over earlier ones:
   with thousands of independent statements that ends in tens of KB of spills
   ... and a compiler-level memory barrier: without it the LDS reads of the state (and of the adjoint state)
   are kept in registers across ALL statements of a chunk -- 2 x 100 doubles at n = 100 -- and the allocator
   spills them to scratch; re-reading LDS per statement is far cheaper */
#define SA_STMT_END asm volatile("" ::: "memory"); __builtin_amdgcn_sched_barrier(0);
#endif

/* Dense matrix-vector block of a callback (generated SA_MATVEC, see symode/codegen.py): out[i] = sum_j M[j*NO+i] v[j]
   with M = a j-major block of the remainder vector (consecutive lanes read consecutive doubles) and v the staged
   state / adjoint state in LDS.  Lane-parallel over the rows: a lane owns rows li, li + G, ...; the four
   interleaved accumulators of the generated association are split between the wavefronts of the workgroup
   (one accumulator each with SA_WAVES = 4), every partial sum goes to LDS and SA_MV(tag, i) adds the four partials
   of row i in the canonical order (a0 + a1) + (a2 + a3).  Replaces n_out * n_in scalar statements that every lane
   used to evaluate redundantly. */
__shared__ double s_mvp[4 * KPW * W_NS];
#define SA_MV(tag, i) ((s_mvp[(0 * KPW + sa_grp()) * W_NS + (i)] + s_mvp[(1 * KPW + sa_grp()) * W_NS + (i)]) + \
                       (s_mvp[(2 * KPW + sa_grp()) * W_NS + (i)] + s_mvp[(3 * KPW + sa_grp()) * W_NS + (i)]))
#define SA_OWNS(slot) (SA_MOD_NWAVES(slot) == sa_wave_index())
template <int NO, int NI>
static __device__ __forceinline__ void sa_matvec_coop(const gdouble *M, const double *v)
{
    static_assert(NO <= W_NS, "matrix-vector block larger than the state vector");
    constexpr int RSL = (NO + G - 1) / G;
    const int lane = (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
    const int li = lane & (G - 1), grp = (KPW == 1) ? 0 : lane / G;
    const bool full = (SA_WAVES > 1) && (s_nwaves == SA_WAVES);     /* (else: one wavefront, sa_k_eval) */
    const int w = full ? sa_wave_index() : 0;
    /* work split: with nw >= 4 wavefronts, wavefront w takes accumulator w % 4 and the row slots r with
       r % (nw / 4) == w / 4; with fewer, its accumulators w, w + nw, ... of every slot.  (nw is SA_WAVES or 1: every
       quotient and remainder below is by a compile-time constant) */
    constexpr int NWF = SA_WAVES > 1 ? SA_WAVES : 1;
    constexpr int ASTEP_F = NWF >= 4 ? 4 : NWF, SGROUPS_F = NWF >= 4 ? NWF / 4 : 1;
    const int astep = full ? ASTEP_F : 1, sgroups = full ? SGROUPS_F : 1, sgrp = full ? (NWF >= 4 ? w / 4 : 0) : 0;
    int row[RSL];
#pragma unroll
    for (int r = 0; r < RSL; r++) row[r] = (r * G + li < NO) ? r * G + li : 0;
    for (int a = full ? w % ASTEP_F : 0; a < 4; a += astep) {
        double acc[RSL];
#pragma unroll
        for (int r = 0; r < RSL; r++) acc[r] = 0.0;
        if (a < NI) {
            /* the matrix entries come from L2 (hundreds of cycles each): fetch a batch of MVB columns for every
               owned row BEFORE the dependent FMA chain consumes them, instead of one load per chain link */
#ifndef SA_MVB
#define SA_MVB 25          /* (7 / 13 / 25 measured on network100: 58.8 / 58.2 / 57.6 ms backward) */
#endif
            constexpr int MVB = SA_MVB;
            constexpr int NT = (NI + 3) / 4;                 /* terms of one accumulator (at most) */
#pragma unroll
            for (int t0 = 0; t0 < NT; t0 += MVB) {
                double mm[MVB][RSL], vv[MVB];
#pragma unroll
                for (int u = 0; u < MVB; u++) {
                    const int j = a + 4 * (t0 + u);
                    const int jc = (t0 + u < NT && j < NI) ? j : a;
                    vv[u] = v[jc];
#pragma unroll
                    for (int r = 0; r < RSL; r++) if (SGROUPS_F == 1 || r % sgroups == sgrp) mm[u][r] = M[jc * NO + row[r]];
                }
#pragma unroll
                for (int u = 0; u < MVB; u++) {
                    const int j = a + 4 * (t0 + u);
                    if (t0 + u < NT && j < NI) {
#pragma unroll
                        for (int r = 0; r < RSL; r++) {
                            if (SGROUPS_F == 1 || r % sgroups == sgrp)
                                acc[r] = (t0 + u == 0) ? mm[u][r] * vv[u] : __builtin_fma(mm[u][r], vv[u], acc[r]);
                        }
                    }
                }
            }
        }
#pragma unroll
        for (int r = 0; r < RSL; r++)
            if ((SGROUPS_F == 1 || r % sgroups == sgrp) && r * G + li < NO) s_mvp[(a * KPW + grp) * W_NS + r * G + li] = acc[r];
    }
    if constexpr (SA_WAVES > 1) sa_barrier();
    else {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
}
#define SA_MATVEC(tag, NO, NI, OFF, VEC) sa_matvec_coop<NO, NI>(prg + (OFF), &VEC(0))

/* Structured matrix callbacks (generated SA_MATFILL): entry(slot) = M[slot] + u[line(slot)].  The N line values are
   evaluated as ordinary statements (split between the wavefronts by SA_OWNS) into LDS; the N*N entries are then
   written by ALL lanes of the instance's lane group / workgroup (coalesced reads of the constant block) instead of
   N*N scalar statements evaluated by every lane; a barrier on either side orders the fill against the line values
   before it and the exception statements after it. */
#define SA_UVEC_BEGIN(tag, N)
#define SA_UVEC_SET(tag, k, v) s_mvp[sa_grp() * W_NS + (k)] = (v)
#define SA_UVEC(tag, k) s_mvp[sa_grp() * W_NS + (k)]
#define SA_STORE_DYN(slot, value) out.put_dyn(slot, value)
static __device__ __forceinline__ void sa_group_sync()
{
    if constexpr (SA_WAVES > 1) sa_barrier();
    else {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
}
template <int N, int AXIS, class SinkT>
static __device__ __forceinline__ double sa_matfill_coop(const gdouble *M, const SinkT &out)
{
    static_assert(N <= W_NS, "matrix block larger than the state vector");
    const int lane = (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
    const int li = lane & (G - 1), grp = (KPW == 1) ? 0 : lane / G;
    const int nw = (SA_WAVES > 1 && s_nwaves == SA_WAVES) ? SA_WAVES : 1;
    const int w = (nw > 1) ? sa_wave_index() : 0;
    sa_group_sync();
    const double *uv = s_mvp + grp * W_NS;
    bool bad = false;
    for (int slot = w * G + li; slot < N * N; slot += nw * G) {
        const double f = M[slot] + uv[AXIS ? slot / N : slot % N];
        out.put_dyn(slot, f);
        bad = bad || (f * 0.0 != 0.0);
    }
    sa_group_sync();
    const uint64_t any = __builtin_amdgcn_ballot_w64(bad);
    const uint64_t mask = (G == 64) ? ~0ull : (((1ull << (G & 63)) - 1ull) << (lane & ~(G - 1)));
    return (any & mask) ? __builtin_nan("") : 0.0;
}
#define SA_MATFILL(tag, N, OFF, AXIS) chk += sa_matfill_coop<N, AXIS>(prg + (OFF), out)

/* Butterfly step: the value of lane (lane ^ 2^B).  Strides 1 and 2 are DPP quad permutes, strides 4 and 8 the DPP
   row_half_mirror / row_mirror patterns (lane 7-i / 15-i instead of i^4 / i^8: inside a SUM or MAX butterfly every
   lane of the partner block already holds that block's total, so any lane of it serves -- same value, same
   association), strides 16 and 32 go through ds_bpermute.  Two VALU moves instead of two LDS-crossbar round trips
   for the four inner stages. */
template <int B>
static __device__ __forceinline__ double sa_xor_lane(double v, int lane)
{
    const uint64_t u = __builtin_bit_cast(uint64_t, v);
    int lo = (int)(uint32_t)u, hi = (int)(uint32_t)(u >> 32);
    if constexpr (B == 0) { lo = __builtin_amdgcn_update_dpp(lo, lo, 0xB1, 0xF, 0xF, false); hi = __builtin_amdgcn_update_dpp(hi, hi, 0xB1, 0xF, 0xF, false); }
    else if constexpr (B == 1) { lo = __builtin_amdgcn_update_dpp(lo, lo, 0x4E, 0xF, 0xF, false); hi = __builtin_amdgcn_update_dpp(hi, hi, 0x4E, 0xF, 0xF, false); }
    else if constexpr (B == 2) { lo = __builtin_amdgcn_update_dpp(lo, lo, 0x141, 0xF, 0xF, false); hi = __builtin_amdgcn_update_dpp(hi, hi, 0x141, 0xF, 0xF, false); }
    else if constexpr (B == 3) { lo = __builtin_amdgcn_update_dpp(lo, lo, 0x140, 0xF, 0xF, false); hi = __builtin_amdgcn_update_dpp(hi, hi, 0x140, 0xF, 0xF, false); }
    else {
        lo = __builtin_amdgcn_ds_bpermute((lane ^ (1 << B)) << 2, lo);
        hi = __builtin_amdgcn_ds_bpermute((lane ^ (1 << B)) << 2, hi);
    }
    return __builtin_bit_cast(double, ((uint64_t)(uint32_t)hi << 32) | (uint64_t)(uint32_t)lo);
}
constexpr int sa_ilog2(int v) { int r = 0; while ((1 << r) < v) r++; return r; }
constexpr int sa_pow2_ge(int v) { int p = 1; while (p < v) p <<= 1; return p; }
template <int B, int E>
static __device__ __forceinline__ double sa_butterfly_sum(double x, int lane)
{
    if constexpr (B < E) { x = x + sa_xor_lane<B>(x, lane); return sa_butterfly_sum<B + 1, E>(x, lane); }
    else return x;
}
template <int P>
static __device__ __forceinline__ double sa_pair_tree(const double *s)
{
    if constexpr (P == 1) return s[0];
    else return sa_pair_tree<P / 2>(s) + sa_pair_tree<P / 2>(s + P / 2);
}

/* Re-rolled sums / outputs of the generated callbacks (codegen.Roller): one term (output) per lane and register
   slot instead of N scalar statements per lane.  SA_SUM is the balanced tree over next_pow2(N) leaves in index
   order: leaf j lives in lane j % G of slot j / G, butterfly over the G lanes of a slot, then the slots pairwise. */
template <int N, class F>
static __device__ __forceinline__ double sa_sum_coop(F term)
{
    constexpr int NSLOT = (N + G - 1) / G, P = sa_pow2_ge(NSLOT);
    const int lane = (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
    const int li = lane & (G - 1);
    double s[P];
#pragma unroll
    for (int r = 0; r < P; r++) {
        if (r < NSLOT) {
            const int j = r * G + li;
            const double x = term(j < N ? j : N - 1);
            s[r] = sa_butterfly_sum<0, sa_ilog2(G)>(j < N ? x : 0.0, lane);
        } else s[r] = 0.0;
    }
    return sa_pair_tree<P>(s);
}
#define SA_SUM(N, term) sa_sum_coop<N>([&](int j_) __attribute__((always_inline)) -> double { return (term); })
template <int N, class F>
static __device__ __forceinline__ double sa_rolled_coop(F body)      /* body(i) evaluates AND stores output i */
{
    constexpr int NSLOT = (N + G - 1) / G;
    const int lane = (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
    const int li = lane & (G - 1);
    bool bad = false;
#pragma unroll
    for (int r = 0; r < NSLOT; r++) {
        const int i = r * G + li;
        if (i < N) { const double v = body(i); bad = bad || (v * 0.0 != 0.0); }
    }
    const uint64_t any = __builtin_amdgcn_ballot_w64(bad);
    const uint64_t mask = (G == 64) ? ~0ull : (((1ull << (G & 63)) - 1ull) << (lane & ~(G - 1)));
    return (any & mask) ? __builtin_nan("") : 0.0;
}
#define SA_ROLLED(N, S0, S1, expr) \
    chk += sa_rolled_coop<N>([&](int i_) __attribute__((always_inline)) -> double { const double v_ = (expr); out.put_dyn((S0) + (S1) * i_, v_); return v_; })
#define SA_UVEC_ROLLED(tag, N, expr) \
    chk += sa_rolled_coop<N>([&](int i_) __attribute__((always_inline)) -> double { const double v_ = (expr); SA_UVEC_SET(tag, i_, v_); return v_; })

/* Lane families of the generated callbacks (symode/codegen.py find_lane_families): a model with M groups whose outputs
   for group f are those of group 0 under the relabelling SA_TAU.  With M == G lanes per instance (SEIR: four age groups
   on the four lanes of a lean group) every lane evaluates ONE member -- its inputs are LDS reads with a lane-dependent
   index, its outputs land in the slots S0 + f -- instead of all M x K outputs in every lane (round-3 / round-4 review:
   "callback outputs distributed over the lanes of a group"); M a multiple of G: the members li, li + G, ... per lane; G a
   multiple of M: member li mod M (lanes beyond M repeat a member: same value into the same slot); otherwise -- and in
   the workgroup-per-instance build -- a plain loop over the members.  The non-finite check of the members is combined
   over the group's lanes. */
static __device__ __forceinline__ double sa_fam_any(double chk)
{
    const int lane = (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
    const uint64_t any = __builtin_amdgcn_ballot_w64(!(chk == 0.0));
    const uint64_t mask = (G == 64) ? ~0ull : (((1ull << (G & 63)) - 1ull) << (lane & ~(G - 1)));
    return (any & mask) ? __builtin_nan("") : 0.0;
}
#define SA_FAM_BEGIN(M) { constexpr bool sa_many_ = (SA_WAVES == 1) && ((M) % G == 0);         /* members li, li + G, ... */ \
    constexpr bool sa_one_ = (SA_WAVES == 1) && !sa_many_ && (G % (M) == 0);                 /* member li mod M     */ \
    constexpr bool sa_dist_ = sa_many_ || sa_one_; \
    const int sa_li_ = (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u)) & (G - 1); \
    const int sa_lo_ = sa_many_ ? sa_li_ : (sa_one_ ? sa_li_ % (M) : 0); \
    const int sa_hi_ = sa_one_ ? sa_lo_ + 1 : (M); \
    for (int sa_f = sa_lo_; sa_f < sa_hi_; sa_f += (sa_many_ ? G : 1)) {
#define SA_F sa_f
#define SA_TAU(j) ((j) == 0 ? sa_f : ((j) == sa_f ? 0 : (j)))
#define SA_FAM_STORE(S0, value) { const double v_ = (value); out.put_dyn((S0) + sa_f, v_); chk += v_ * 0.0; }
#define SA_FAM_END } if (sa_dist_) chk = sa_fam_any(chk); }

#include SA_PROBLEM_HEADER
#include "sa_device_abi.h"
#include "sa_common.h"

static_assert(NS == W_NS && NQ == W_NQ, "SA_BUILD_NS / SA_BUILD_NQ do not match the generated header");
static_assert(NS <= 8 * G && NQ <= 8 * G && NS >= 1 && NS <= 128, "at most eight register slots per vector");

#define RS ((NS + G - 1) / G)                  /* register slots of a state vector */
#define RQ (NQ > 0 ? (NQ + G - 1) / G : 1)     /* register slots of a quadrature vector */
constexpr int ilog2_c(int v) { int r = 0; while ((1 << r) < v) r++; return r; }
#define LOG2G ilog2_c(G)
#define GMASK (G == 64 ? ~0ull : ((1ull << G) - 1ull))
/* arena records: the divided-difference table of the point {order, dt, T[6], Y[6][n]}, or with -DSA_COMPACT_TRAJ what
   CVODES itself stores per step, {order, t, y[n]} (the table is then rebuilt in the backward pass when the index
   moves: bdf_kernels.hip has the same switch) */
#if defined(SA_COMPACT_TRAJ) && !defined(SA_HERMITE)
#define SA_COMPACT 1
#define TREC (NS + 2)
#define TREC_T 1
#define TREC_Y 2
#else
#define SA_COMPACT 0
#define TREC (8 + 6 * NS)
#define TREC_T 2
#define TREC_Y 8
#endif
#define SA_NAN __builtin_bit_cast(double, (uint64_t)0x7ff8000000000000ULL)
constexpr int pow2_ge(int v) { int p = 1; while (p < v) p <<= 1; return p; }
/* workspace (doubles per instance): saved Jacobian + callback output vector */
#define WS_SJ 0
#define WS_OUT (NS * NS)
#define WS_SMALL0 (NS * NS + ((NS > NQ ? NS : NQ) + 7) / 8 * 8)
#ifdef SA_SENS
/* forward-sensitivity builds (lane groups only): per instance additionally the fresh Jacobian and df/dp of the
   sensitivity right-hand side; then, per WAVEFRONT, the sensitivity vectors [vector][parameter][slot][lane] */
#define WS_JS WS_SMALL0
#define WS_DP (WS_SMALL0 + NS * NS)
#define WS_SMALL (WS_SMALL0 + NS * NS + NQD_ * NS)
#define NQD_ (NQ > 0 ? NQ : 1)
#define WS_DOUBLES (WS_SMALL + SV_COUNT * NQD_ * RS * G)
#else
#define WS_SMALL WS_SMALL0
#define WS_DOUBLES WS_SMALL0
#endif
/* workspace of instance `inst`: the wavefront's block starts at its first instance, the per-instance parts come
   first (WS_SMALL doubles each), the wavefront-wide sensitivity block after them */
static __device__ __forceinline__ double *ws_inst(double *ws, int inst)
{
    return ws + (int64_t)(inst / KPW * KPW) * WS_DOUBLES + (int64_t)(inst % KPW) * WS_SMALL;
}

/* ---- cross-lane primitives (the wave is always converged when these run) ---- */
DEV int lane_id() { return (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u)); }

DEV double shfl_d(double v, int src_lane)
{
    const uint64_t u = __builtin_bit_cast(uint64_t, v);
    const uint32_t lo = (uint32_t)__builtin_amdgcn_ds_bpermute(src_lane << 2, (int)(uint32_t)u);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_ds_bpermute(src_lane << 2, (int)(uint32_t)(u >> 32));
    return __builtin_bit_cast(double, ((uint64_t)hi << 32) | (uint64_t)lo);
}
DEV int shfl_i(int v, int src_lane) { return __builtin_amdgcn_ds_bpermute(src_lane << 2, v); }

/* value of lane `src` (wave-uniform index) */
DEV double readlane_d(double v, int src)
{
    const uint64_t u = __builtin_bit_cast(uint64_t, v);
    const uint32_t lo = __builtin_amdgcn_readlane((uint32_t)u, src);
    const uint32_t hi = __builtin_amdgcn_readlane((uint32_t)(u >> 32), src);
    return __builtin_bit_cast(double, ((uint64_t)hi << 32) | (uint64_t)lo);
}

DEV uint64_t readlane_u64(double v, int src)
{
    const uint64_t u = __builtin_bit_cast(uint64_t, v);
    const uint32_t lo = __builtin_amdgcn_readlane((uint32_t)u, src);
    const uint32_t hi = __builtin_amdgcn_readlane((uint32_t)(u >> 32), src);
    return ((uint64_t)hi << 32) | (uint64_t)lo;
}

DEV void lds_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

/* output sinks of the generated callbacks (all lanes hold the same value) */
struct VecOut {             /* vector-valued callbacks -> the instance's LDS output vector */
    int base;
    template <int S> __device__ __forceinline__ void put(double x) const { s_out[base + S] = x; }
    __device__ __forceinline__ void put_dyn(int slot, double x) const { s_out[base + slot] = x; }
};
struct MatOut {             /* n x n callbacks -> the instance's LDS matrix (slot = col * n + row) */
    int base;
    template <int S> __device__ __forceinline__ void put(double x) const { s_A[base + S] = x; }
    __device__ __forceinline__ void put_dyn(int slot, double x) const { s_A[base + slot] = x; }
};
struct GMatOut {            /* lean lane groups: n x n callbacks -> the saved Jacobian in the workspace (every lane of the
                               group holds the same value and writes it: one transaction per group) */
    gdouble *p;
    template <int S> __device__ __forceinline__ void put(double x) const { p[S] = x; }
    __device__ __forceinline__ void put_dyn(int slot, double x) const { p[slot] = x; }
};

/* ------------------------------------------------------------------------------------ */
template <bool BWD>
struct Cw {
    int lane;                         /* lane in the wavefront */
    int li, gbase;                    /* lane within its instance's group, first lane of the group */
    int abase, vbase, pbase, kbase, obase;   /* the group's slices of s_A / s_y,s_lam / s_ps / s_piv / s_out */
    double zn[QMAX + 1][RS], znQ[QMAX + 1][RQ], zsave[RS], zsaveQ[RQ];
    double ewt[RS], acor[RS], tempv[RS], ftemp[RS], y[RS], ytmp[RS], atol[RS];
#ifdef SA_CONSTRAINTS
    double cons[RS];                  /* CVodeSetConstraints entries of the lane's components */
    int constr;
#endif
    double ewtQ[RQ], acorQ[RQ], tempvQ[RQ];
    double inv_piv[RS];               /* 1/pivot of the rows the lane owns */
    int nswaps;                       /* row exchanges of the current factorisation */
    double *sj, *obuf;                /* workspace: saved Jacobian, callback output vector */
    const double *pr;
    double rtol, rtolQ, atolQ;
    double tn, h, hprime, hscale, eta, etamax, hu;
    int q, qprime, L, qwait, qu;
    double tau[7], tq[6], l[7];
    double rl1, gamma, gammap, gamrat, crate, delp, acnrm, saved_tq5;
    double etaq, etaqm1, etaqp1, tstop;
    int nst, nfe, nje, nsetups, nni, ncfn, netf, nfQe, netfQ, nstlp, nstlj;
    int jcur, nls_jcur;
    /* stored trajectory (backward): current divided-difference record, own components */
    const double *traj;
    int64_t trow;
    int np;
    double tfinal;
    int ilast, newdata, have_last, cur_idx;
    double last_t, tlo, thi, tlo2;
#if !SA_TAB_LDS
    double tab_hdr[8];                /* order, dt, T[6] */
    double tabY[QMAX + 1][RS];
#endif
#if SA_LEAN
    double lu[NS][RS];                /* LU factors of I - gamma*J, rows IDX(r) of every column: live in registers from
                                         the factorisation to the next one (no LDS matrix) */
#endif
#ifdef SA_HERMITE
    double f0[RS];                    /* f(t0, y0) of the first stored point */
#endif
    int n_interp, n_rebuild;
#ifdef SA_SENS
    /* forward sensitivities (Solver(sens_mode=...), reference solver.py:360-392): the NQ sensitivity Nordsieck arrays
       and work vectors live in the workspace (SV(m, vector, parameter, slot)), streamed through registers phase by phase */
    double *sws;
    const double *pbar;
    double crateS, delpS, acnrmS;
    int sensi, ism, nfSe, nniS, ncfnS, netfS, nsetupsS;
#endif
#ifdef SA_WAVE_PROFILE
    int64_t prof[8];                  /* 10 ns ticks: rhs, quad, jac, getrf, getrs, matrix copy */
#endif
};

#if defined(SA_WAVE_PROFILE) && !defined(SA_WAVE_PROFILE_PHASES)   /* tuning builds: section timers -> stats 9..15 */
#define PROF_T0 const int64_t prof_t0 = (int64_t)wall_clock64();
#define PROF_ADD(m, k) (m).prof[k] += (int64_t)wall_clock64() - prof_t0;
#else
#define PROF_T0
#define PROF_ADD(m, k)
#endif
/* -DSA_WAVE_PROFILE -DSA_WAVE_PROFILE_PHASES: the same slots time the phases of a step attempt instead:
   0 pre-step (weights, norm), 1 adjust + predict + cvSet, 2 interpolation, 3 Newton pass (callbacks, LU and solves
   included), 4 error test + quadrature, 5 complete + prepare next step */
#if defined(SA_WAVE_PROFILE) && defined(SA_WAVE_PROFILE_PHASES)
#define PH_T0 int64_t ph_t0 = (int64_t)wall_clock64();
#define PH_ADD(m, k) { const int64_t now_ = (int64_t)wall_clock64(); (m).prof[k] += now_ - ph_t0; ph_t0 = now_; }
#else
#define PH_T0
#define PH_ADD(m, k)
#endif

#define IDX(m, r) ((r) * G + (m).li)

/* pairwise (balanced-tree) sum of P = 2^k slot totals */
template <int P>
DEV double slot_tree(const double (&s)[P])
{
    if constexpr (P == 1) return s[0];
    else {
        double half[P / 2];
        SFOR(i, 0, P / 2) half[i] = s[2 * i] + s[2 * i + 1]; SEND
        return slot_tree<P / 2>(half);
    }
}

/* sum over all lanes and slots: xor-butterfly per slot, then the slot totals pairwise */
template <int NSLOT>
DEV double wave_sum(int lane, const double (&v)[NSLOT])
{
    constexpr int P = pow2_ge(NSLOT);
    double s[P];
    SFOR(r, 0, P) {
        if constexpr (r < NSLOT) {
            s[r] = sa_butterfly_sum<0, LOG2G>(v[r], lane);
        } else {
            s[r] = 0.0;
        }
    } SEND
    return slot_tree<P>(s);
}

DEV double wave_max(int lane, double x)
{
    SFOR(b, 0, LOG2G) { const double o = sa_xor_lane<b>(x, lane); x = x > o ? x : o; } SEND
    return x;
}

template <bool BWD>
DEV double wrms_n(const Cw<BWD> &m, const double (&x)[RS], const double (&w)[RS])
{
    double sq[RS];
    SFOR(r, 0, RS) { const double prod = (IDX(m, r) < NS) ? x[r] * w[r] : 0.0; sq[r] = prod * prod; } SEND
    return sqrt(wave_sum<RS>(m.lane, sq) / NS);
}

template <bool BWD>
DEV double wrms_q(const Cw<BWD> &m, const double (&x)[RQ], const double (&w)[RQ])
{
    if constexpr (NQ == 0) return 0.0;
    double sq[RQ];
    SFOR(r, 0, RQ) { const double prod = (IDX(m, r) < NQ) ? x[r] * w[r] : 0.0; sq[r] = prod * prod; } SEND
    return sqrt(wave_sum<RQ>(m.lane, sq) / (NQ > 0 ? NQ : 1));
}

template <bool BWD>
DEV double quad_update_norm(const Cw<BWD> &m, double old_nrm, const double (&xQ)[RQ])
{
    const double qnrm = wrms_q(m, xQ, m.ewtQ);
    return old_nrm > qnrm ? old_nrm : qnrm;
}

template <bool BWD>
DEV int ewt_set(const Cw<BWD> &m, const double (&ycur)[RS], double (&w)[RS])
{
    double bad = 0.0;
    SFOR(r, 0, RS) {
        const double v = FMA(m.rtol, fabs(ycur[r]), m.atol[r]);
        bad = (IDX(m, r) < NS && v <= 0.0) ? 1.0 : bad;
        w[r] = 1.0 / v;
    } SEND
    return wave_max(m.lane, bad) > 0.0 ? -1 : 0;
}

template <bool BWD>
DEV int ewtQ_set(const Cw<BWD> &m, const double (&qcur)[RQ], double (&w)[RQ])
{
    double bad = 0.0;
    SFOR(r, 0, RQ) {
        const double v = FMA(m.rtolQ, fabs(qcur[r]), m.atolQ);
        bad = (IDX(m, r) < NQ && v <= 0.0) ? 1.0 : bad;
        w[r] = 1.0 / v;
    } SEND
    return wave_max(m.lane, bad) > 0.0 ? -1 : 0;
}

/* ---- stored trajectory: records as in bdf_kernels.hip ({order, dt, T[6], Y[6][n]} per point) ---- */
template <bool BWD>
DEV double point_time(const Cw<BWD> &m, int s) { return m.traj[(int64_t)s * m.trow + TREC_T]; }

#if SA_COMPACT
/* the table CVApolynomialGetY builds at index indx from the stored points indx, indx-1, .. indx-order (newest first):
   hdr = {order, dt, T[0..5]}, Y[j] = divided differences scaled by dt^j -- the operation order of the oracle
   (factor = dt / (T[j] - T[j-i]); Y[j] = factor * (Y[j] - Y[j-1])), all loads in flight together, unused columns zero.
   (Measured and not kept: the lanes of a group touching, ahead of these loads, the points the next 4 / 8 index moves
   will add -- retired with the loads, so nothing stays outstanding: SEIR backward 52.0 / 52.9 against 52.0 ms.) */
template <bool BWD>
DEV void load_points(const Cw<BWD> &m, int indx, double (&hdr)[8], double (&Y)[QMAX + 1][RS])
{
    const gdouble *r = (const gdouble *)(m.traj + (int64_t)indx * m.trow);
    const int order = (int)r[0];
    double hT[QMAX + 1];
    SFOR(j, 0, (QMAX) + 1) {
        const gdouble *rj = (const gdouble *)(m.traj + (int64_t)(indx - j > 0 ? indx - j : 0) * m.trow);
        hT[j] = rj[TREC_T];
        SFOR(s, 0, RS) {
            const double v = rj[TREC_Y + (IDX(m, s) < NS ? IDX(m, s) : 0)];
            Y[j][s] = (j <= order) ? v : 0.0;
        } SEND
    } SEND
    const double dt = fabs(hT[0] - hT[1]);
    SFOR(i, 1, (QMAX) + 1) {
        SFOR_DOWN(j, QMAX, 1) {
            if constexpr (j >= i) {
                if (j <= order) {
                    const double factor = SA_TABLE_DIV(dt, hT[j] - hT[j - i]);
                    SFOR(s, 0, RS) Y[j][s] = factor * (Y[j][s] - Y[j - 1][s]); SEND
                }
            }
        } SEND
    } SEND
    hdr[0] = (double)order; hdr[1] = dt;
    SFOR(j, 0, (QMAX) + 1) hdr[2 + j] = hT[j]; SEND
}
#endif

template <bool BWD>
DEV int interp_y(Cw<BWD> &m, double t)
{
    if (m.have_last && t == m.last_t) return CV_SUCCESS;
    m.n_interp++;
    int newpoint = 0, indx;
    if (m.newdata) {
        m.ilast = m.np - 1; newpoint = 1; m.newdata = 0;
        m.tlo = point_time(m, m.ilast - 1); m.thi = point_time(m, m.ilast);
        m.tlo2 = (m.ilast >= 2) ? point_time(m, m.ilast - 2) : m.tlo;
    }
    const int ilast = m.ilast;
    const bool to_left = (t - m.tlo) < 0.0;
    const bool to_right = (t - m.thi) > 0.0;
    indx = ilast;
    if (to_left) {
        newpoint = 1;
        double tprev = m.tlo, tcur = m.thi;
        for (;;) {
            if (indx == 0) break;
            if ((t - tprev) <= 0.0) {
                indx--;
                tcur = tprev;
                if (indx > 0) tprev = (indx == ilast - 1) ? m.tlo2 : point_time(m, indx - 1);
            } else break;
        }
        m.ilast = (indx == 0) ? 1 : indx;
        if (indx == 0) {
            m.tlo = tcur; m.thi = point_time(m, 1);
            if (fabs(t - m.tlo) > FUZZ_FACTOR_ADJ * UROUND) return CV_GETY_BADT;
        } else {
            m.tlo = tprev; m.thi = tcur;
        }
    } else if (to_right) {
        newpoint = 1;
        double tcur = m.thi, tprev = m.tlo;
        for (;;) {
            if (indx >= m.np - 1) break;
            if ((t - tcur) > 0.0) {
                indx++;
                tprev = tcur;
                tcur = point_time(m, indx);
            } else break;
        }
        m.ilast = indx;
        m.tlo = tprev; m.thi = tcur;
        if ((t - m.thi) > FUZZ_FACTOR_ADJ * UROUND * (fabs(m.tfinal) + 1.0)) return CV_GETY_BADT;
    }
    m.have_last = 1;
    m.last_t = t;
    if (indx == 0) {
        SFOR(r, 0, RS) m.ytmp[r] = (IDX(m, r) < NS) ? m.traj[TREC_Y + (IDX(m, r) < NS ? IDX(m, r) : 0)] : 0.0; SEND
        return CV_SUCCESS;
    }
#ifdef SA_HERMITE
    {   /* CVAhermiteGetY (see the oracle): tab_hdr[2..3] = t0, t1; tabY[0..3] = y0, y0', Y0, Y1 of the interval */
        if (newpoint) {
            m.n_rebuild++;
            m.cur_idx = indx;
            const double *r0 = m.traj + (int64_t)(indx - 1) * m.trow, *r1 = m.traj + (int64_t)indx * m.trow;
            m.tab_hdr[2] = r0[2]; m.tab_hdr[3] = r1[2];
            const double delta = m.tab_hdr[3] - m.tab_hdr[2];
            SFOR(s, 0, RS) {
                const int c = IDX(m, s) < NS ? IDX(m, s) : 0;
                const double y0 = r0[8 + c], yd0 = r0[8 + NS + c], y1 = r1[8 + c], yd1 = r1[8 + NS + c];
                const double dy = y1 - y0;
                m.tabY[0][s] = y0; m.tabY[1][s] = yd0;
                m.tabY[2][s] = FMA(-delta, yd0, dy);
                m.tabY[3][s] = FMA(delta, yd1 + yd0, -2.0 * dy);
            } SEND
            if (indx == m.ilast) m.tlo2 = (indx >= 2) ? point_time(m, indx - 2) : m.tlo;
        }
        const double delta = m.tab_hdr[3] - m.tab_hdr[2];
        const double factor1 = t - m.tab_hdr[2];
        double factor2 = factor1 / delta;
        factor2 = factor2 * factor2;
        const double factor3 = factor2 * (t - m.tab_hdr[3]) / delta;
        SFOR(s, 0, RS) {
            double acc = FMA(factor1, m.tabY[1][s], m.tabY[0][s]);
            acc = FMA(factor2, m.tabY[2][s], acc);
            acc = FMA(factor3, m.tabY[3][s], acc);
            m.ytmp[s] = (IDX(m, s) < NS) ? acc : 0.0;
        } SEND
        return CV_SUCCESS;
    }
#endif
#if SA_TAB_LDS
    double *tab = s_tab + (m.lane / G) * W_TRECP;
    if (newpoint) {
        m.n_rebuild++;
        m.cur_idx = indx;
        const gdouble *r = (const gdouble *)(m.traj + (int64_t)indx * m.trow);
        /* the group copies the record (8 + 6n doubles) arena -> LDS, all loads in flight before the first store.
           (Measured and not kept, SEIR: touching the lines of the next-left record ahead of time -- at the move itself
           every function call then waits for the touch, interp 7.8 -> 10.5 ms; after the attempt's last callback,
           8 k call-free cycles ahead of the next move: 9.0 ms, the whole backward kernel 63.1 -> 65.3 ms.) */
#if SA_COMPACT
        {   /* rebuild from the order + 1 points ending at indx: every lane its own components, the times group-uniform */
            double hdr[8], Y[QMAX + 1][RS];
            load_points(m, indx, hdr, Y);
            lds_sync();
            if (m.li == 0) { SFOR(f, 0, 8) tab[f] = hdr[f]; SEND }
            SFOR(j, 0, (QMAX) + 1) { SFOR(s2, 0, RS) { if (IDX(m, s2) < NS) tab[8 + j * NS + IDX(m, s2)] = Y[j][s2]; } SEND } SEND
            lds_sync();
        }
#else
        constexpr int NCP = (W_TREC + G - 1) / G;
        double cp[NCP];
        SFOR(u, 0, NCP) { const int f = u * G + m.li; cp[u] = r[f < W_TREC ? f : 0]; } SEND
        lds_sync();
        SFOR(u, 0, NCP) { const int f = u * G + m.li; if (f < W_TREC) tab[f] = cp[u]; } SEND
        lds_sync();
#endif
        if (tab[0] > (double)indx) return CV_GETY_BADT;
        if (indx == m.ilast) m.tlo2 = tab[4];
    }
    {
        double hdr[8], ty[QMAX + 1][RS];
        SFOR(f, 0, 8) hdr[f] = tab[f]; SEND
        SFOR(i, 0, (QMAX) + 1) { SFOR(s, 0, RS) ty[i][s] = tab[8 + i * NS + (IDX(m, s) < NS ? IDX(m, s) : 0)]; SEND } SEND
        const int order = (int)hdr[0];
        const double inv_dt = SA_TABLE_DIV(1.0, hdr[1]);
        double cvals[QMAX + 1];
        cvals[0] = 1.0;
        SFOR(i, 0, QMAX) cvals[i + 1] = (i < order) ? cvals[i] * (t - hdr[2 + i]) * inv_dt : 0.0; SEND
        SFOR(s, 0, RS) {
            double acc = cvals[0] * ty[0][s];
            SFOR(i, 1, (QMAX) + 1) acc = FMA(cvals[i], ty[i][s], acc); SEND
            m.ytmp[s] = (IDX(m, s) < NS) ? acc : 0.0;
        } SEND
    }
    return CV_SUCCESS;
#else
    if (newpoint) {
        m.n_rebuild++;
        m.cur_idx = indx;
#if SA_COMPACT
        load_points(m, indx, m.tab_hdr, m.tabY);
#else
        const double *r = m.traj + (int64_t)indx * m.trow;
        SFOR(f, 0, 8) m.tab_hdr[f] = r[f]; SEND
        SFOR(j, 0, (QMAX) + 1) {
            SFOR(s, 0, RS) {
                const int c = IDX(m, s) < NS ? IDX(m, s) : 0;
                m.tabY[j][s] = r[8 + j * NS + c];
            } SEND
        } SEND
#endif
        if (m.tab_hdr[0] > (double)indx) return CV_GETY_BADT;
        if (indx == m.ilast) m.tlo2 = m.tab_hdr[4];
    }
    {
        const int order = (int)m.tab_hdr[0];
        const double inv_dt = SA_TABLE_DIV(1.0, m.tab_hdr[1]);
        double cvals[QMAX + 1];
        cvals[0] = 1.0;
        SFOR(i, 0, QMAX) cvals[i + 1] = (i < order) ? cvals[i] * (t - m.tab_hdr[2 + i]) * inv_dt : 0.0; SEND
        SFOR(s, 0, RS) {
            double acc = cvals[0] * m.tabY[0][s];
            SFOR(i, 1, (QMAX) + 1) acc = FMA(cvals[i], m.tabY[i][s], acc); SEND
            m.ytmp[s] = (IDX(m, s) < NS) ? acc : 0.0;
        } SEND
    }
    return CV_SUCCESS;
#endif
}

/* ---- callbacks: stage the inputs in LDS, evaluate, fetch the owned outputs ---- */
template <bool BWD>
DEV void stage_inputs(const Cw<BWD> &m, const double (&ymine)[RS])
{
    lds_sync();
    SFOR(r, 0, RS) {
        if (IDX(m, r) < NS) {
            if constexpr (BWD) { s_y[m.vbase + IDX(m, r)] = m.ytmp[r]; s_lam[m.vbase + IDX(m, r)] = ymine[r]; }
            else s_y[m.vbase + IDX(m, r)] = ymine[r];
        }
    } SEND
    lds_sync();
}

template <bool BWD, int NSLOT, int N>
DEV void fetch_output(const Cw<BWD> &m, double (&out)[NSLOT])
{
    lds_sync();
    SFOR(r, 0, NSLOT) out[r] = (IDX(m, r) < N) ? s_out[m.obase + (IDX(m, r) < N ? IDX(m, r) : 0)] : 0.0; SEND
    lds_sync();
}

/* every wavefront of the workgroup runs this for the same command; SA_CHUNK_CALL picks its chunks */
template <bool BWD>
DEV int run_callback(int cmd, double t, const double *pr, double *obuf)
{
    if (cmd == CMD_RHS) {
        if constexpr (BWD) return sa_adj_rhs(t, nullptr, nullptr, nullptr, pr, VecOut{sa_grp() * W_NOUTP});
        else return sa_rhs(t, nullptr, nullptr, pr, VecOut{sa_grp() * W_NOUTP});
    }
    if (cmd == CMD_QUAD) return sa_quad_rhs(t, nullptr, nullptr, nullptr, pr, VecOut{sa_grp() * W_NOUTP});
    if constexpr (SA_LEAN) {
        gdouble *sjp = (gdouble *)(obuf - WS_OUT + WS_SJ);
        if constexpr (BWD) return sa_adj_jac(t, nullptr, nullptr, pr, GMatOut{sjp});
        else return sa_jac(t, nullptr, nullptr, pr, GMatOut{sjp});
    } else {
        if constexpr (BWD) return sa_adj_jac(t, nullptr, nullptr, pr, MatOut{sa_grp() * NS * NS});
        else return sa_jac(t, nullptr, nullptr, pr, MatOut{sa_grp() * NS * NS});
    }
}

/* wavefront 0: publish the command (the inputs are already staged), evaluate, collect */
template <bool BWD>
DEV int dispatch(Cw<BWD> &m, int cmd, double t)
{
    if constexpr (SA_WAVES > 1) {
        if (m.li == 0) { s_cmd = cmd; s_targ = t; }
        sa_barrier();
    }
    int rc = run_callback<BWD>(cmd, t, m.pr, m.obuf);
    if constexpr (SA_WAVES > 1) {
        if (m.li == 0) s_rc[0] = rc;
        sa_barrier();
        SFOR(w, 1, SA_WAVES) rc |= s_rc[w]; SEND
    }
    return rc;
}

/* coordinates of a lane for the LU routines (workers build one without an integrator state) */
struct Grp {
    int lane, li, gbase, abase, kbase, wave;
};
DEV int getrf_coop(const Grp &g, double (&inv_piv)[(W_NS + G - 1) / G], int &nswaps);
/* LDS arrays the factorisation works on, as explicit LDS-address-space pointers: inside a noinline function the
   compiler reaches a __shared__ variable that only such functions use through a per-kernel offset TABLE in global
   memory -- one dependent global load per access group, several per elimination step.  The kernels (where the
   addresses are constants) build this block and pass it by value. */
typedef __attribute__((address_space(3))) double lds_f64;
typedef __attribute__((address_space(3))) int lds_i32;
typedef __attribute__((address_space(3))) uint8_t lds_u8;
typedef __attribute__((address_space(3))) int64_t lds_i64;
struct LuLds {
    lds_f64 *A, *col, *invp;
    lds_u8 *piv;
    lds_i32 *ier, *nswaps, *info, *pub;
    lds_i64 *prof;
};
static __device__ __attribute__((noinline)) void setup_lu_regs(int wave, int lane, double c, int from_saved, double *sj, LuLds L);
static __device__ __forceinline__ void setup_lu_regs_body(int wave, int lane, double c, int from_saved, double *sj, LuLds L);
#define LU_RING_SLOTS SA_WAVES
static __device__ __forceinline__ LuLds lu_lds();

template <bool BWD>
DEV void worker_loop(const double *pr, double *obuf)
{
    const int lane = lane_id(), wave = sa_wave_index();
    for (;;) {
        sa_barrier();
        const int cmd = s_cmd;
        const double t = s_targ;
        if (cmd == CMD_EXIT) break;
        if (cmd == CMD_GETRF) {
            /* A CALL on purpose, also here.  As a call the function saves and restores its ~100 callee-saved vector
               registers on every factorisation in every wavefront (11.8 GB of scratch writes per backward launch of
               config 5, profiles/r04_network100_pmc.txt) although the workers have nothing live.  Inlining the body
               here (-DSA_LU_INLINE_WORKERS: scratch per lane 256 -> 192 B, three quarters of those writes gone) was
               measured in round 5 and is SLOWER: network100 15.84 -> 15.44 k solves/s (backward 55.05 -> 56.43 ms,
               forward 9.51 -> 9.75): the scratch round trip overlaps with the first loads of the factorisation, the
               second copy of the function costs instruction-cache misses and 60 more scalar spills in the kernel. */
#ifdef SA_LU_INLINE_WORKERS
            setup_lu_regs_body(wave, lane, t, s_flag, obuf - WS_OUT + WS_SJ, lu_lds());
#else
            setup_lu_regs(wave, lane, t, s_flag, obuf - WS_OUT + WS_SJ, lu_lds());
#endif
        } else {
            const int rc = run_callback<BWD>(cmd, t, pr, obuf);
            if (lane == 0) s_rc[wave] = rc;
        }
        sa_barrier();
    }
}

template <bool BWD>
DEV void release_workers(const Cw<BWD> &m)
{
    if constexpr (SA_WAVES > 1) {
        if (m.li == 0) s_cmd = CMD_EXIT;
        sa_barrier();
    }
}

template <bool BWD>
DEV int cv_f(Cw<BWD> &m, double t, const double (&ymine)[RS], double (&out)[RS])
{
    m.nfe++;
    PROF_T0
    stage_inputs(m, ymine);
    const int rc = dispatch(m, CMD_RHS, t);
    fetch_output<BWD, RS, NS>(m, out);
    PROF_ADD(m, 0)
    return rc;
}

template <bool BWD>
DEV int cv_fQ(Cw<BWD> &m, double t, const double (&ymine)[RS], double (&out)[RQ])
{
    m.nfQe++;
    PROF_T0
    stage_inputs(m, ymine);
    const int rc = dispatch(m, CMD_QUAD, t);
    fetch_output<BWD, RQ, (NQ > 0 ? NQ : 1)>(m, out);
    PROF_ADD(m, 1)
    return rc;
}

template <bool BWD>
DEV int cv_jac(Cw<BWD> &m, double t, const double (&ymine)[RS])        /* Jacobian -> s_A */
{
    PROF_T0
    stage_inputs(m, ymine);
    const int rc = dispatch(m, CMD_JAC, t);
    lds_sync();
    PROF_ADD(m, 2)
    return rc;
}

/* ---- row-distributed dense LU in LDS (denseGETRF / denseGETRS semantics) ---- */
#define AL(i, j) s_A[g.abase + (j) * NS + (i)]
#ifndef LU_BATCH
#define LU_BATCH 8
#endif
#define GETRS_DEPTH 4

/* barrier between the phases of an elimination step: the workgroup when worker wavefronts take part,
   otherwise the LDS ordering of the (possibly diverged) wavefront */
DEV void lu_sync()
{
    if constexpr (SA_WAVES > 1) sa_barrier();
    else lds_sync();
}

/* LU of the instance's LDS matrix.  With worker wavefronts (G = 64) ALL wavefronts of the workgroup take
   part: every wavefront repeats the pivot search and the scaling of column k on identical data (identical
   decisions, no communication), the trailing columns are split between the wavefronts, one workgroup
   barrier per elimination step; wavefront 0 writes the scaled column back one step late, when nobody
   reads the unscaled entries any more.  With G < 64 lanes per instance the group works alone. */
DEV int getrf_coop(const Grp &g, double (&inv_piv)[RS], int &nswaps)
{
    nswaps = 0;
    double lcol[RS];
    SFOR(r, 0, RS) lcol[r] = 0.0; SEND
    for (int k = 0; k < NS; k++) {
        if (g.wave == 0 && k > 0) {
            SFOR(r, 0, RS) { const int i = r * G + g.li; if (i > k - 1 && i < NS) AL(i, k - 1) = lcol[r]; } SEND
            if constexpr (SA_WAVES == 1) lds_sync();
        }
        /* pivot: first row i >= k with the largest |a(i,k)| (strict '>' scan order of denseGETRF).
           I - gamma*J is close to diagonally dominant, so usually no row beats the diagonal: one
           ballot settles that case, the arg-max butterfly only runs when some lane disagrees. */
        double akk = AL(k, k);
        double best = fabs(akk);
        int bi = k;
        bool beaten = false;
        double cand[RS], colv[RS];      /* column k below the diagonal: raw values and magnitudes */
        SFOR(r, 0, RS) {
            const int i = r * G + g.li;
            colv[r] = (i > k && i < NS) ? AL(i, k) : 0.0;
            cand[r] = (i > k && i < NS) ? fabs(colv[r]) : -1.0;
            beaten = beaten || (cand[r] > best);
        } SEND
        if (((__builtin_amdgcn_ballot_w64(beaten) >> g.gbase) & GMASK) != 0) {
            best = -1.0;
            bi = 1 << 20;
            SFOR(r, 0, RS) {
                const int i = r * G + g.li;
                const double v = (i == k) ? fabs(AL(k, k)) : cand[r];
                if (i >= k && i < NS && v > best) { best = v; bi = i; }
            } SEND
            SFOR(b, 0, LOG2G) {
                const double ov = shfl_d(best, g.lane ^ (1 << b));
                const int oi = shfl_i(bi, g.lane ^ (1 << b));
                const bool take = (ov > best) || (ov == best && oi < bi);
                best = take ? ov : best;
                bi = take ? oi : bi;
            } SEND
        }
        const int l = bi;               /* identical in every lane of the group */
        if (g.wave == 0 && g.li == 0) s_piv[g.kbase + k] = (uint8_t)l;
        if (best == 0.0) return k + 1;
        if (l != k) {                   /* exchange rows k and l, one column per lane */
            nswaps++;
            lu_sync();
            for (int c = g.wave * G + g.li; c < NS; c += G * SA_WAVES) {
                const double x = AL(k, c), y = AL(l, c);
                AL(k, c) = y;
                AL(l, c) = x;
            }
            lu_sync();
            akk = AL(k, k);             /* rows moved: fetch the column again */
            SFOR(r, 0, RS) { const int i = r * G + g.li; colv[r] = (i > k && i < NS) ? AL(i, k) : 0.0; } SEND
        }
        const double mult = 1.0 / akk;
        SFOR(r, 0, RS) {
            const int i = r * G + g.li;
            inv_piv[r] = (i == k) ? mult : inv_piv[r];
            lcol[r] = (i > k && i < NS) ? colv[r] * mult : 0.0;
        } SEND
        /* elimination: this wavefront's batches of LU_BATCH columns, all reads of a batch before its writes */
        for (int j = k + 1 + g.wave * LU_BATCH; j < NS; j += LU_BATCH * SA_WAVES) {
            double akj[LU_BATCH], x[LU_BATCH][RS];
            SFOR(u, 0, LU_BATCH) {
                const bool on = (j + u) < NS;
                akj[u] = on ? AL(k, on ? j + u : j) : 0.0;
                SFOR(r, 0, RS) {
                    const int i = r * G + g.li;
                    x[u][r] = (on && i > k && i < NS) ? AL(i, j + u) : 0.0;
                } SEND
            } SEND
            SFOR(u, 0, LU_BATCH) {
                if (akj[u] != 0.0) {
                    SFOR(r, 0, RS) {
                        const int i = r * G + g.li;
                        if ((j + u) < NS && i > k && i < NS) AL(i, j + u) = FMA(-akj[u], lcol[r], x[u][r]);
                    } SEND
                }
            } SEND
        }
        lu_sync();
    }
    return 0;
}

/* the addresses go through an empty asm: otherwise interprocedural constant propagation puts the __shared__ globals
   back into the callee -- and with them the offset-table loads */
template <class T>
static __device__ __forceinline__ T *lds_opaque(T *p)
{
    uint32_t a = (uint32_t)(uintptr_t)p;
    asm volatile("" : "+s"(a));
    return (T *)(uintptr_t)a;
}
/* ---- LU of a lane group with the matrix in REGISTERS (G < 64, small systems: config 4) ----
 * The 64/G instances of a wavefront factorise at different times, so the wavefront pays for a factorisation in
 * nearly every iteration of its attempt loop even though an instance needs one in a third of its steps (SEIR: the
 * LDS version's 43 k cycles per call were the largest single item of the backward kernel).  Here lane li of the
 * group loads rows li, li + G of all columns (NS*RS doubles), eliminates without touching LDS -- the pivot-row entry
 * of a column is a ds_bpermute from its home lane, every lane scales its own rows' multipliers (the reciprocal of
 * the pivot is recomputed per lane: no publication, no barrier) -- and writes the factors back for the triangular
 * solves.  Rows are never moved: an exchange relabels (logical index per register slot, as in setup_lu_regs).  The
 * steps are unrolled (k is a compile-time index).  Branch-free trailing update: multipliers of finished rows are
 * zero; denseGETRF's skip of columns with a zero pivot-row entry is dropped (a - 0*l == a).  Same operations on the
 * same values as getrf_coop / denseGETRF otherwise, hence the same factors (test_row_exchanges_in_the_dense_lu). */
#ifndef LU_GROUP_REGS_MAX
#define LU_GROUP_REGS_MAX 40                   /* NS*RS doubles per lane up to which the register version is used */
#endif
DEV int getrf_group_regs(const Grp &g, double (&inv_piv)[RS], int &nswaps)
{
    double a[NS][RS];
    int logpos[RS];
    SFOR(j, 0, NS) {
        SFOR(r, 0, RS) { const int i = r * G + g.li; a[j][r] = AL(i < NS ? i : 0, j); } SEND
    } SEND
    SFOR(r, 0, RS) {
        const int i = r * G + g.li;
        logpos[r] = (i < NS) ? i : -1;
        if (i >= NS) { SFOR(j, 0, NS) a[j][r] = 0.0; SEND }
    } SEND
    nswaps = 0;
    int ier = 0;
    /* home (lane of the group, register slot) of logical row K, identical in every lane of the group */
#define LUG_HOME(K, HL, HS) do { HL = 0; HS = 0;                                                                \
        SFOR(r, 0, RS) {                                                                                        \
            const uint32_t grp = (uint32_t)((__builtin_amdgcn_ballot_w64(logpos[r] == (K)) >> g.gbase) & GMASK); \
            if (grp != 0) { HS = r; HL = __builtin_ctz(grp); }                                                  \
        } SEND } while (0)
    SFOR(k, 0, NS) {
        int hl, hs;
        LUG_HOME(k, hl, hs);
        double dsel = a[k][0];
        SFOR(r, 1, RS) dsel = (hs == r) ? a[k][r] : dsel; SEND
        const double akk = shfl_d(dsel, g.gbase + hl);
        /* pivot: first (lowest logical index) row i >= k with the largest |a(i,k)| */
        double best = fabs(akk);
        int bi = k;
        bool beaten = false;
        double cand[RS];
        SFOR(r, 0, RS) {
            cand[r] = (logpos[r] > k) ? fabs(a[k][r]) : -1.0;
            beaten = beaten || (cand[r] > best);
        } SEND
        if (((__builtin_amdgcn_ballot_w64(beaten) >> g.gbase) & GMASK) != 0) {
            best = -1.0;
            bi = 1 << 20;
            SFOR(r, 0, RS) {
                const double v = (logpos[r] == k) ? fabs(akk) : cand[r];
                if (logpos[r] >= k && (v > best || (v == best && logpos[r] < bi))) { best = v; bi = logpos[r]; }
            } SEND
            SFOR(b, 0, LOG2G) {
                const double ov = shfl_d(best, g.lane ^ (1 << b));
                const int oi = shfl_i(bi, g.lane ^ (1 << b));
                const bool take = (ov > best) || (ov == best && oi < bi);
                best = take ? ov : best;
                bi = take ? oi : bi;
            } SEND
        }
        const int l = bi;                   /* identical in every lane of the group */
        if (g.li == 0) s_piv[g.kbase + k] = (uint8_t)l;
        ier = (ier == 0 && best == 0.0) ? k + 1 : ier;          /* keep going (results unused): no exit edges */
        double apiv = akk;
        if (l != k) {                       /* row exchange = relabelling */
            nswaps++;
            SFOR(r, 0, RS) { const int lp = logpos[r]; logpos[r] = (lp == l) ? k : ((lp == k) ? l : lp); } SEND
            LUG_HOME(k, hl, hs);
            double psel = a[k][0];
            SFOR(r, 1, RS) psel = (hs == r) ? a[k][r] : psel; SEND
            apiv = shfl_d(psel, g.gbase + hl);
        }
        const double mult = 1.0 / apiv;
        double lc[RS];
        SFOR(r, 0, RS) {
            inv_piv[r] = (r * G + g.li == k) ? mult : inv_piv[r];
            const bool below = logpos[r] > k;
            lc[r] = below ? a[k][r] * mult : 0.0;
            a[k][r] = below ? lc[r] : a[k][r];
        } SEND
        SFOR(j, k + 1, NS) {
            double src = a[j][0];
            SFOR(r, 1, RS) src = (hs == r) ? a[j][r] : src; SEND
            const double akj = shfl_d(src, g.gbase + hl);
            SFOR(r, 0, RS) a[j][r] = FMA(-akj, lc[r], a[j][r]); SEND
        } SEND
    } SEND
#undef LUG_HOME
    SFOR(j, 0, NS) {
        SFOR(r, 0, RS) { if (logpos[r] >= 0) AL(logpos[r], j) = a[j][r]; } SEND
    } SEND
    return ier;
}

/* ---- Newton matrix set-up + LU by the whole workgroup, matrix in REGISTERS (SA_WAVES > 1, G = 64) ----
 * M = I + c*J (c = -gamma) is built and factorised without touching LDS in the elimination.  The blocked right-looking
 * LU (exchange rows, triangular panel solve, rank-4 update) with the element-wise operation order of denseGETRF:
 * columns are owned in PANELS of LU_NB = 4 consecutive columns, dealt round robin to the wavefronts -- wavefront w
 * holds the panels p = pr * SA_WAVES + w (pr < LU_NPR) in the register columns pr * LU_NB .. pr * LU_NB + 3, lane l the
 * rows l, l + 64 (2 * LU_NC doubles per lane).
 *   - A panel is factorised INSIDE its owner: four elimination steps (pivot check, reciprocal, scaling, update of
 *     the panel's later columns) in straight-line code, no LDS and no synchronisation in between.  The diagonal is the
 *     pivot in all but a few factorisations of I - gamma*J: the check is one ballot; only if some row beats the
 *     diagonal does the arg-max butterfly run and are the two rows EXCHANGED (readlane + select) in the panel.
 *   - The owner publishes (LDS ring) the four multiplier columns as they stand after the whole panel -- i.e. with
 *     the panel's later exchanges applied, zero on and above the diagonal, so nobody needs a mask -- and the four
 *     pivot rows, then bumps a counter.  There is NO barrier per panel (round 3: one per COLUMN, 100 at n = 100):
 *     the wavefronts run as a dataflow pipeline on that counter, see the loop.
 *   - Every wavefront applies the panel's row exchanges to its other columns (rare), then the four steps to its
 *     trailing columns, step-outer / column-inner: pivot-row entry = v_readlane of its own register column (row k
 *     already carries the steps before k), one FMA per owned entry.  Exchanging rows l > k, k' > k before instead of
 *     after the update of step k changes no value (each row's arithmetic is the same, the multipliers are published
 *     in the exchanged frame), so every entry receives a(i,j) = fma(-a(k,j), l(i,k), a(i,j)) for k = 0, 1, 2 ... in
 *     this order with l(i,k) = a(i,k) * (1 / pivot): denseGETRF's operations on the same values in the same order,
 *     hence the same factors bit for bit (test_row_exchanges_in_the_dense_lu[wave], every network test).
 * J comes from the saved copy in the workspace (from_saved) or from LDS where the Jacobian callback just wrote it
 * (and is saved on the way); the factors end up in LDS (s_A) for the triangular solves of wavefront 0, the
 * reciprocal pivots in s_invp.
 * History (profiles/r03_network100_sections.txt, r04_network100_lu.txt): round 3 -- one column per barrier, 1 970
 * cycles per elimination step, half of them the owner's serial chain with the other three wavefronts waiting: 73 us
 * per 100 x 100 factorisation.  Panels with a barrier each: 45 us.  Dataflow: see the profile. */
#if SA_WAVES > 1
#ifndef LU_NB
#define LU_NB 4
#endif
#define LU_INFO (LU_NB + 4)                 /* ints per ring slot: LU_NB pivot rows, #exchanges, zero-pivot step + 1, padding */
#define LU_NPANEL ((NS + LU_NB - 1) / LU_NB)
#define LU_NPR ((LU_NPANEL + SA_WAVES - 1) / SA_WAVES)
#define LU_NC (LU_NPR * LU_NB)
/* register slot (rows 64 * slot .. 64 * slot + 63) that holds the pivot rows / diagonal entries of the panels of round PR */
#define LU_SLOT_OF_BLOCK(PR) ((RS == 1) ? 0 : ((((PR) * SA_WAVES * LU_NB) >> 6) < RS ? (((PR) * SA_WAVES * LU_NB) >> 6) : RS - 1))
static_assert(RS <= 2 && 64 % (LU_NB * SA_WAVES) == 0 && (SA_WAVES & (SA_WAVES - 1)) == 0,
              "the rows of a panel round share one register slot; the ring of published panels has SA_WAVES slots");
__shared__ __attribute__((aligned(16))) double s_col[LU_RING_SLOTS][RS * 64 * LU_NB];      /* ring of published panels */
__shared__ double s_invp[W_NS];
__shared__ __attribute__((aligned(16))) int s_luinfo[LU_RING_SLOTS * LU_INFO];     /* per ring slot: 4 pivot rows, #exchanges, zero-pivot step + 1 */
__shared__ int s_luier, s_lunswaps, s_lupub;
#ifdef SA_WAVE_PROFILE
__shared__ int64_t s_luprof[12];           /* wavefront 0, cycles: panel factorisation, waiting, trailing update, whole function (ticks /
                                              cycles), load + form, first barrier, write-back, last barrier */
#endif
#if defined(SA_WAVE_PROFILE) && defined(SA_LU_PROFILE_SEGMENTS)     /* (the inner timers cost ~800 cycles per panel themselves) */
#define LUP_T(x) const int64_t x = (int64_t)__builtin_readcyclecounter();
#define LUP_ADD(k, a, b) if (wave == 0 && lane == 0) L.prof[k] += (b) - (a);
#else
#define LUP_T(x)
#define LUP_ADD(k, a, b)
#endif
#define LU_SING 0x100000
/* place of row 64 * r + lane of column kk of the published panel in ring slot `slot`: a column's rows are contiguous
   (lane stride 8 bytes: every ds_read / ds_write_b64 of a wavefront is bank-conflict free; with the four columns of a row
   side by side -- 32 bytes from lane to lane -- each access was an 8-way conflict, ~600 cycles per panel on the owner's chain) */
#define LU_PIDX(slot, r, kk) ((((slot) * LU_NB + (kk)) * RS + (r)) * 64 + lane)

static __device__ __forceinline__ LuLds lu_lds()
{
    LuLds L;
    L.A = lds_opaque((lds_f64 *)s_A); L.col = lds_opaque((lds_f64 *)&s_col[0][0]); L.invp = lds_opaque((lds_f64 *)s_invp);
    L.piv = lds_opaque((lds_u8 *)s_piv);
    L.ier = lds_opaque((lds_i32 *)&s_luier); L.nswaps = lds_opaque((lds_i32 *)&s_lunswaps);
    L.info = lds_opaque((lds_i32 *)&s_luinfo[0]);
    L.pub = lds_opaque((lds_i32 *)&s_lupub);
#ifdef SA_WAVE_PROFILE
    L.prof = lds_opaque((lds_i64 *)s_luprof);
#else
    L.prof = nullptr;
#endif
    return L;
}

/* wait until `want` panels are published.  Fence-to-fence synchronisation THROUGH AN ATOMIC (with a plain
   volatile counter the ring accesses were formally a data race that only the AMDGPU lowering made work): the owner
   writes the panel, issues a workgroup-scope release fence and stores the counter atomically (lu_publish); a reader
   loads it atomically until it is large enough, then issues the acquire fence the panel reads are ordered behind.
   Same instructions as before. */
static __device__ __forceinline__ void lu_wait(lds_i32 *pub, int want)
{
    /* (one wavefront per SIMD: a spinning wavefront takes nothing from anybody; with two per SIMD it yields) */
    while (__builtin_amdgcn_readfirstlane(__hip_atomic_load(pub, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)) < want) {
        if (SA_WAVES > 4) __builtin_amdgcn_s_sleep(1);
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}
static __device__ __forceinline__ void lu_publish(lds_i32 *pub, int count)     /* after the release fence, by ONE lane */
{
    __hip_atomic_store(pub, count, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

static __device__ __forceinline__ void lu_pin(double &x) { asm volatile("" : "+v"(x)); }
/* max(x, |y|) as the one instruction it is (fmax() adds a canonicalising v_max_f64 x, x per operand); a NaN operand loses */
static __device__ __forceinline__ double vmax_abs(double x, double y)
{
    double r;
    asm("v_max_f64 %0, %1, |%2|" : "=v"(r) : "v"(x), "v"(y));
    return r;
}
/* value of register slot `slot` (wave-uniform) of a column */
#define LU_SEL(col, slot) (RS == 1 ? (col)[0] : ((slot) == 0 ? (col)[0] : (col)[RS - 1]))
/* exchange rows (slot s1, lane l1) and (slot s2, lane l2) of a register column (rare path) */
#define LU_SWAP_ROWS(col, s1, l1, s2, l2) do {                                                              \
        const double v1_ = readlane_d(LU_SEL(col, s1), l1), v2_ = readlane_d(LU_SEL(col, s2), l2);        \
        SFOR(r_, 0, RS) {                                                                                   \
            (col)[r_] = (r_ == (s1) && lane == (l1)) ? v2_ : ((r_ == (s2) && lane == (l2)) ? v1_ : (col)[r_]); \
        } SEND } while (0)

/* noinline for wavefront 0 on purpose: the 2*LU_NC matrix registers of a lane must not compete with its integrator
   state (inlined, the pair spilled ~1.6 KB per lane to scratch); results come back through LDS.  The worker
   wavefronts inline the body (worker_loop). */
static __device__ __attribute__((noinline)) void setup_lu_regs(int wave, int lane, double c, int from_saved, double *sj, LuLds L)
{
    setup_lu_regs_body(wave, lane, c, from_saved, sj, L);
}
static __device__ __forceinline__ void setup_lu_regs_body(int wave, int lane, double c, int from_saved, double *sj, LuLds L)
{
    double a[LU_NC][RS];
    LUP_T(t_in)
#ifdef SA_WAVE_PROFILE
    const int64_t w_in = (int64_t)wall_clock64();
#endif
    wave = __builtin_amdgcn_readfirstlane(wave);            /* wave-uniform by construction: let the compiler know */
    /* register column cc <-> matrix column ((cc / LU_NB) * SA_WAVES + wave) * LU_NB + cc % LU_NB.  All loads of the
       matrix are issued back to back (clamped index instead of a branch per entry) */
#define LU_COL(cc) ((((cc) / LU_NB) * SA_WAVES + wave) * LU_NB + (cc) % LU_NB)
    typedef __attribute__((address_space(1))) double glb_f64;
    glb_f64 *sjg = (glb_f64 *)sj;
    /* Instruction count matters here too (56 entries per lane): the row index is clamped once per register slot, the
       column once per register column on the scalar unit; padding rows / columns are zeroed through the factor
       they are multiplied with (their loads hit a valid address: finite values); the diagonal of register column cc
       lies in the slot of its round (compile-time), only there is it looked for. */
    int ri[RS];
    double cr[RS];                                          /* c for the rows that exist, 0 for the padding rows */
    SFOR(r, 0, RS) {
        const int i = r * 64 + lane;
        ri[r] = i < NS ? i : NS - 1;
        cr[r] = (i < NS) ? c : 0.0;
    } SEND
    if (from_saved) {
        SFOR(cc, 0, LU_NC) {
            const int j = LU_COL(cc), jc = j < NS ? j : NS - 1;
            glb_f64 *colp = sjg + jc * NS;
            SFOR(r, 0, RS) a[cc][r] = colp[ri[r]]; SEND
        } SEND
    } else {
        SFOR(cc, 0, LU_NC) {
            const int j = LU_COL(cc), jc = j < NS ? j : NS - 1;
            lds_f64 *colp = L.A + jc * NS;
            SFOR(r, 0, RS) a[cc][r] = colp[ri[r]]; SEND
        } SEND
        SFOR(cc, 0, LU_NC) {
            const int j = LU_COL(cc);
            if (j < NS) {                                   /* (wave-uniform) */
                glb_f64 *colp = sjg + j * NS;
                SFOR(r, 0, RS) {
                    if ((r + 1) * 64 <= NS) colp[r * 64 + lane] = a[cc][r];
                    else if (r * 64 + lane < NS) colp[r * 64 + lane] = a[cc][r];
                } SEND
            }
        } SEND
    }
    SFOR(cc, 0, LU_NC) {
        const int j = LU_COL(cc);
        constexpr int SD = LU_SLOT_OF_BLOCK(cc / LU_NB);    /* slot of the diagonal entry of this column */
        double cj[RS];
        SFOR(r, 0, RS) cj[r] = (j < NS) ? cr[r] : 0.0; SEND             /* (scalar condition) */
        SFOR(r, 0, RS) {
            const double v = a[cc][r];
            if constexpr (r == SD) a[cc][r] = (lane == (j & 63) && j < NS) ? FMA(c, v, 1.0) : v * cj[r];
            else a[cc][r] = v * cj[r];
        } SEND
    } SEND
    if (wave == 0 && lane == 0) { (*L.ier) = 0; (*L.pub) = 0; }
    int nswaps = 0, ier = 0;
#ifdef SA_WAVE_PROFILE
    asm volatile("" :: "v"(a[0][0]), "v"(a[LU_NC - 1][RS - 1]));
#endif
    LUP_T(t_ld)
    sa_barrier();
#ifdef SA_LU_PROFILE_TIMELINE
    const int64_t t_loop = (int64_t)__builtin_readcyclecounter();
#else
    LUP_T(t_loop)
#endif
    LUP_ADD(5, t_in, t_ld) LUP_ADD(6, t_ld, t_loop)
    /* DATAFLOW over the panels p = 0, 1, ... (p = pr * SA_WAVES + o; the round pr -- which register columns the owner
       works on -- is unrolled, the SA_WAVES panels of a round are a run-time loop), no barrier inside:
         every wavefront, for p = 0, 1, ...:   wait until panel p-1 is published; read it; apply its row exchanges;
             the OWNER of p:  apply p-1 to the four columns of p, factorise them, publish (ring slot p mod SA_WAVES,
                              then the counter), ...
             everyone:        ... apply p-1 to the other trailing columns.
       The chain  publish(p-1) -> update of four columns -> panel factorisation -> publish(p)  is the critical path;
       the trailing updates of all wavefronts run beside it (with a barrier per panel the three other wavefronts
       idled through every panel factorisation and the owner through their updates).  A wavefront cannot run more
       than SA_WAVES - 1 panels ahead of the slowest one (it needs that one's next panel), hence the ring.
       No exit edges (an exit edge makes the register allocator copy the whole register matrix on every iteration):
       panels past the end or after a zero pivot run as no-ops (zero multipliers).
       A lone wavefront issues ONE instruction of any kind per four cycles (tools/ubench_issue.hip: v_fma_f64,
       v_readlane_b32, s_nop, s_add all 4.1 cycles; a dependent FMA chain 5.1), so what counts below is the NUMBER of
       instructions, scalar ones included.  The rows of a whole round live in one register slot S (compile-time):
       slots below S hold finished rows (no work at all), slot S is masked by the lane, slots above S take part with
       every row. */
#define LU_SLOT(PR) LU_SLOT_OF_BLOCK(PR)
#ifndef LU_GC
#define LU_GC 4
#endif
    static_assert(LU_NB % LU_GC == 0, "panel width in whole column groups");
    /* the trailing update with panel p-1 of the register columns [C0, C1): step-outer, column-inner in groups of LU_GC
       columns -- the broadcasts of a group, then its FMAs, a scheduling barrier (left alone the scheduler hoists every
       broadcast of a step to the front, runs out of scalar registers and spills them through v_writelane /
       v_readlane: three lane operations per value instead of one).  Branch-free: the multiplier of a row that takes
       no part in a step is zero; slots below SP hold finished rows only and are skipped.  (denseGETRF skips a column
       whose pivot-row entry is zero; a - 0*l equals a -- only the sign of a zero entry can differ -- so the factors
       compare equal and no result changes.)  The results are pinned at the end of a group: the rows of the slots above
       SP are not read again before the end of the factorisation, and the compiler otherwise sinks their whole FMA
       chains below everything else, keeping every broadcast value alive (spilled lane by lane) until then. */
#define LU_UPD_GROUP(SP, C0, C1, KK) {                                                                              \
        double akj_[LU_GC];                                                                                           \
        SFOR(cc, C0, C1) akj_[cc - (C0)] = readlane_d(a[cc][SP], plp + (KK)); SEND                                    \
        SFOR(cc, C0, C1) { SFOR(r, SP, RS) a[cc][r] = FMA(-akj_[cc - (C0)], lc[KK][r], a[cc][r]); SEND } SEND         \
        SFOR(cc, C0, C1) { SFOR(r, SP, RS) lu_pin(a[cc][r]); SEND } SEND                                              \
        __builtin_amdgcn_sched_barrier(0); }
#define LU_UPD_SAME(SP) SFOR(kk, 0, LU_NB) {                                                                        \
        SFOR(g, 0, LU_NB / LU_GC) LU_UPD_GROUP(SP, pr * LU_NB + g * LU_GC, pr * LU_NB + g * LU_GC + LU_GC, kk) SEND } SEND
#define LU_UPD_MAIN(SP) SFOR(kk, 0, LU_NB) {                                                                        \
        SFOR(g, 0, (LU_NC - (pr + 1) * LU_NB + LU_GC - 1) / LU_GC) {                                                  \
            constexpr int c0 = (pr + 1) * LU_NB + g * LU_GC, c1 = (c0 + LU_GC < LU_NC) ? c0 + LU_GC : LU_NC;          \
            LU_UPD_GROUP(SP, c0, c1, kk)                                                                              \
        } SEND } SEND
    /* the published panel q (ring slot q mod SA_WAVES): words -> word[], multiplier columns of the slots >= SP -> lc */
    /* (measured and not kept: reading the counter and the panel's data in ONE batch per spin turn -- one LDS round trip
       less on the chain in theory, 58.65 against 58.4 ms in practice) */
#define LU_READ(SP, Q)                                                                                              \
        const int slot_ = (Q) & (SA_WAVES - 1);                                                                       \
        int nex_ = L.info[slot_ * LU_INFO + LU_NB], ierp_ = L.info[slot_ * LU_INFO + LU_NB + 1];                      \
        SFOR(r, SP, RS) { SFOR(kk, 0, LU_NB) lc[kk][r] = L.col[LU_PIDX(slot_, r, kk)]; SEND } SEND \
        nex_ = __builtin_amdgcn_readfirstlane(nex_); ierp_ = __builtin_amdgcn_readfirstlane(ierp_);
    /* The row exchanges of a published panel (first row kq, pivot rows in slot SP) in the register columns [C0, C1)
       and [C2, C3): the (at most four) exchanges are composed into ONE gather map per lane and slot -- src[r] = the
       position (64 * slot + lane) whose value belongs here afterwards -- and every column is gathered once through
       ds_bpermute.  Rare, straight-line (a run-time loop over the exchanges would carry the whole register matrix
       through it, and the compiler pays for that with a copy of the matrix in front of the loop on EVERY pass).
       Rows of the slots below SP are finished and never move. */
#define LU_GATHER_MAP(SP, kq) int src_[RS];                                                                         \
        SFOR(r, 0, RS) src_[r] = r * 64 + lane; SEND                                                                  \
        SFOR(kk, 0, LU_NB) {                                                                                          \
            const int kl_ = ((kq) + kk) & 63, l_ = word[kk] & 0xff, ls_ = (RS == 1) ? 0 : (l_ >> 6), ll_ = l_ & 63;   \
            const int ck_ = __builtin_amdgcn_readlane(src_[SP], kl_);                                                 \
            const int cl_ = __builtin_amdgcn_readlane(ls_ == (SP) ? src_[SP] : src_[RS - 1], ll_);                    \
            SFOR(r, SP, RS) {                                                                                         \
                src_[r] = (r == (SP) && lane == kl_) ? cl_ : ((r == ls_ && lane == ll_) ? ck_ : src_[r]);             \
            } SEND                                                                                                    \
        } SEND
#define LU_GATHER_COL(SP, col) {                                                                                    \
        double nv_[RS];                                                                                               \
        SFOR(r, SP, RS) {                                                                                             \
            nv_[r] = shfl_d((col)[SP], src_[r] & 63);                                                                 \
            SFOR(s2, SP + 1, RS) { const double t_ = shfl_d((col)[s2], src_[r] & 63); nv_[r] = ((src_[r] >> 6) == s2) ? t_ : nv_[r]; } SEND \
        } SEND                                                                                                        \
        SFOR(r, SP, RS) (col)[r] = nv_[r]; SEND }
    /* ... of panel q = p - 1 (owner oq), applied by every OTHER wavefront to all its columns before it uses the panel;
       (the common case costs two scalar compares: the owner publishes the number of exchanges and the zero-pivot flag) */
#define LU_SWAPS(SP, kq, oq)                                                                                        \
        if (ierp_ != 0 && wave != (oq)) ier = (ier == 0) ? ierp_ : ier;                                               \
        if (nex_ != 0 && wave != (oq)) {                                                                              \
            nswaps += nex_;                                                                                           \
            SFOR(kk, 0, LU_NB) word[kk] = __builtin_amdgcn_readfirstlane(L.info[slot_ * LU_INFO + kk]); SEND                \
            LU_GATHER_MAP(SP, kq)                                                                                     \
            SFOR(cc, 0, LU_NC) LU_GATHER_COL(SP, a[cc]) SEND                                                          \
        }
    SFOR(pr, 0, LU_NPR) {
        constexpr int S = LU_SLOT(pr);                          /* register slot of this round's rows */
        constexpr int SQ = pr > 0 ? LU_SLOT(pr - 1) : S;        /* ... of the round before (panel p-1 when o == 0) */
        /* (panels past the last column do not exist: the last round may be shorter) */
        constexpr int NO = (LU_NPANEL - pr * SA_WAVES) < SA_WAVES ? (LU_NPANEL - pr * SA_WAVES) : SA_WAVES;
#pragma nounroll
        for (int o = 0; o < NO; o++) {
            const int p = pr * SA_WAVES + o, k0 = p * LU_NB;
            const int pl0 = k0 & 63, plp = (k0 - LU_NB) & 63;   /* lane of the first row of panel p / of panel p-1 */
            const int op = (o + SA_WAVES - 1) & (SA_WAVES - 1); /* owner of panel p-1 */
            double lc[LU_NB][RS];
            int word[LU_NB];
            SFOR(kk, 0, LU_NB) { word[kk] = 0; SFOR(r, 0, RS) lc[kk][r] = 0.0; SEND } SEND
            const bool first = (pr == 0) && (o == 0);           /* (no panel before the first) */
            const bool prev_round = (S != SQ) && (o == 0);      /* panel p-1 lives in the slot of the round before */
            LUP_T(t_a)
            if (!first) {
                lu_wait(L.pub, p);
                if (prev_round) { LU_READ(SQ, p - 1) LU_SWAPS(SQ, k0 - LU_NB, op) }
                else { LU_READ(S, p - 1) LU_SWAPS(S, k0 - LU_NB, op) }
            }
            LUP_T(t_b)
            int own_word[LU_NB], own_swaps = 0;
            SFOR(kk, 0, LU_NB) own_word[kk] = 0; SEND
            if (wave == o) {
                if (!first) { if (prev_round) { LU_UPD_SAME(SQ) } else { LU_UPD_SAME(S) } }
                LUP_T(t_b1)
                LUP_ADD(9, t_b, t_b1)
                int pword[LU_NB];
                double mults[LU_NB];
                constexpr bool PARTIAL = (NS % LU_NB) != 0;     /* (a last panel with columns past n exists) */
                /* FAST PATH.  The owner's chain -- update of its four columns, these four steps, publication -- is the
                   critical path of the whole factorisation, and it is paid in instructions (four cycles each).  So the
                   four steps first run SPECULATIVELY as if every diagonal entry were an acceptable non-zero pivot (it
                   is, in all but a few factorisations of I - gamma*J): no per-step branch, the rows below the diagonal
                   under one lane mask (no selects), zero / beaten pivots only recorded.  If anything was recorded, the
                   panel is restored from a copy and redone by the general code below -- same operations, same values in
                   the case that counts. */
                bool general = PARTIAL || (ier != 0);
                if (!general) {
                    double keep[LU_NB][RS];
                    SFOR(kk, 0, LU_NB) { SFOR(r, S, RS) keep[kk][r] = a[pr * LU_NB + kk][r]; SEND } SEND
                    /* Costs that do not show in the instruction count (tools/ubench_issue.hip): a VALU compare consumed by
                       the scalar unit stalls the wavefront ~20 cycles, an IEEE division is a 74-cycle chain.  So: "some
                       row beats the diagonal" is accumulated on the VALU (max of |a(i,k)| - |a(k,k)|, one compare at the
                       end), the pivot's sanity test is integer work on the scalar unit, and the reciprocal is the division's
                       own expansion without the scaling / fix-up instructions -- v_rcp_f64 and six FMAs, the same bits as
                       1.0 / x whenever nothing would be scaled (exponent within 2^-500 .. 2^500, checked: anything else,
                       zero included, goes to the general code; 2^30 random operands compared in the micro-benchmark). */
                    double over = 0.0;                          /* max(|a(i,k)| - |a(k,k)|) over the rows below the diagonal */
                    int odd = 0;                                /* sign bit set: some pivot's exponent outside 2^-500 .. 2^500 */
                    SFOR(kk, 0, LU_NB) {
                        constexpr int kc = pr * LU_NB + kk;
                        const uint64_t abits = readlane_u64(a[kc][S], pl0 + kk);
                        const double akk = __builtin_bit_cast(double, abits);
                        const int ex = (int)((uint32_t)(abits >> 52) & 0x7ffu);
                        odd |= (ex - 523) | (1523 - ex);
                        double mult = __builtin_amdgcn_rcp(akk), e_ = FMA(-akk, mult, 1.0);
                        mult = FMA(mult, e_, mult); e_ = FMA(-akk, mult, 1.0);
                        mult = FMA(mult, e_, mult); e_ = FMA(-akk, mult, 1.0);
                        mult = FMA(e_, mult, mult);
                        mults[kk] = mult;
                        pword[kk] = (k0 + kk) & 0xff;
                        double akj[LU_NB];
                        SFOR(jj, kk + 1, LU_NB) akj[jj] = readlane_d(a[pr * LU_NB + jj][S], pl0 + kk); SEND
                        double big = 0.0;                       /* largest |a(i,k)| below the diagonal, this lane */
                        SFOR(r, S + 1, RS) {
                            big = vmax_abs(big, a[kc][r]);
                            a[kc][r] = a[kc][r] * mult;
                            SFOR(jj, kk + 1, LU_NB) a[pr * LU_NB + jj][r] = FMA(-akj[jj], a[kc][r], a[pr * LU_NB + jj][r]); SEND
                        } SEND
                        if (lane > pl0 + kk) {                  /* the rows of slot S below the diagonal */
                            big = vmax_abs(big, a[kc][S]);
                            a[kc][S] = a[kc][S] * mult;
                            SFOR(jj, kk + 1, LU_NB) a[pr * LU_NB + jj][S] = FMA(-akj[jj], a[kc][S], a[pr * LU_NB + jj][S]); SEND
                        }
                        over = vmax_abs(big - fabs(akk), over); /* (over >= 0 always; a NaN entry is ignored like the comparison ignores it) */
                    } SEND
                    if (odd < 0 || __builtin_amdgcn_ballot_w64(over > 0.0) != 0) {
                        general = true;
                        SFOR(kk, 0, LU_NB) { SFOR(r, S, RS) a[pr * LU_NB + kk][r] = keep[kk][r]; SEND } SEND
                    }
                }
                if (general)
                SFOR(kk, 0, LU_NB) {
                    const int k = k0 + kk;
                    constexpr int kc = pr * LU_NB + kk;
                    /* a step past the end (k >= n) or after a zero pivot runs with a unit pivot: nothing changes, and
                       no branch joins here (a join copies the panel's register columns).  The pivot is a scalar (the
                       same in every lane by construction): its zero test and the bookkeeping that hangs on it stay
                       on the scalar unit. */
                    const bool valid = (ier == 0) && (k0 < NS) && (!PARTIAL || k < NS);
                    uint64_t abits = readlane_u64(a[kc][S], pl0 + kk);
                    double akk = __builtin_bit_cast(double, abits);
                    /* the diagonal stays the pivot unless a row below it is strictly larger */
                    bool beaten = (lane > pl0 + kk) && (fabs(a[kc][S]) > fabs(akk));        /* (slot S; above: every row) */
                    SFOR(r, S + 1, RS) beaten = beaten || (fabs(a[kc][r]) > fabs(akk)); SEND
                    int l = k;
                    if (valid && __builtin_amdgcn_ballot_w64(beaten) != 0) {
                        /* pivot: first (lowest index) row i >= k with the largest |a(i,k)| */
                        double best = -1.0;
                        int bi = 1 << 20;
                        SFOR(r, S, RS) {
                            const int i = r * 64 + lane;
                            const double v = fabs(a[kc][r]);
                            if (i >= k && (v > best || (v == best && i < bi))) { best = v; bi = i; }
                        } SEND
#pragma nounroll
                        for (int b = 0; b < 6; b++) {
                            const double ov = shfl_d(best, lane ^ (1 << b));
                            const int oi = shfl_i(bi, lane ^ (1 << b));
                            const bool take = (ov > best) || (ov == best && oi < bi);
                            best = take ? ov : best;
                            bi = take ? oi : bi;
                        }
                        l = __builtin_amdgcn_readfirstlane(bi);
                        if (l != k) {
                            nswaps++;
                            own_swaps++;
                            const int ls = (RS == 1) ? 0 : (l >> 6), ll = l & 63;
                            SFOR(jj, 0, LU_NB) LU_SWAP_ROWS(a[pr * LU_NB + jj], S, pl0 + kk, ls, ll); SEND
                            abits = readlane_u64(a[kc][S], pl0 + kk);
                            akk = __builtin_bit_cast(double, abits);
                        }
                    }
                    const bool nonzero = (abits << 1) != 0;
                    if (valid && !nonzero) {            /* (rare; nothing below changes anything after it) */
                        ier = k + 1;
                        if (lane == 0) (*L.ier) = k + 1;
                    }
                    const bool ok = valid && nonzero;
                    const double mult = 1.0 / __builtin_bit_cast(double, ok ? abits : (uint64_t)0x3ff0000000000000ull);
                    pword[kk] = l & 0xff;
                    own_word[kk] = l & 0xff;
                    mults[kk] = mult;
                    double lcp[RS];
                    {
                        const bool on = ok && (lane > pl0 + kk);
                        const double v = a[kc][S] * mult;
                        lcp[S] = on ? v : 0.0;
                        a[kc][S] = on ? v : a[kc][S];
                    }
                    SFOR(r, S + 1, RS) { a[kc][r] = a[kc][r] * mult; lcp[r] = ok ? a[kc][r] : 0.0; } SEND
                    SFOR(jj, kk + 1, LU_NB) {           /* the panel's later columns */
                        const double akj = readlane_d(a[pr * LU_NB + jj][S], pl0 + kk);
                        SFOR(r, S, RS) a[pr * LU_NB + jj][r] = FMA(-akj, lcp[r], a[pr * LU_NB + jj][r]); SEND
                    } SEND
                } SEND
                /* publish: the multiplier columns as they stand now (the panel's later exchanges applied): slot S
                   masked by the lane, the slots above as they are (a step that did not run -- past the end: the
                   column is zero; after a zero pivot: the factorisation has failed, nobody uses the result); the
                   pivot rows, the number of exchanges, the zero-pivot flag; then -- release -- the counter */
                const int slot = p & (SA_WAVES - 1);
                LUP_T(t_b2)
                LUP_ADD(10, t_b1, t_b2)
                SFOR(kk, 0, LU_NB) {
                    L.col[LU_PIDX(slot, S, kk)] = (lane > pl0 + kk) ? a[pr * LU_NB + kk][S] : 0.0;
                } SEND
                SFOR(r, S + 1, RS) {
                    SFOR(kk, 0, LU_NB) L.col[LU_PIDX(slot, r, kk)] = a[pr * LU_NB + kk][r]; SEND
                } SEND
                if (lane == 0) {
                    SFOR(kk, 0, LU_NB) L.info[slot * LU_INFO + kk] = pword[kk]; SEND
                    L.info[slot * LU_INFO + LU_NB] = own_swaps;
                    L.info[slot * LU_INFO + LU_NB + 1] = ier;
                }
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
                if (lane == 0) {
                    lu_publish(L.pub, p + 1);
#ifdef SA_LU_PROFILE_TIMELINE       /* cycles from the first barrier to the publication of panel (workgroup index mod #panels) */
                    if (p == (int)(blockIdx.x % LU_NPANEL)) L.prof[11] += (int64_t)__builtin_readcyclecounter() - t_loop;
#endif
                    /* (off the chain: the pivots are read by wavefront 0 only after the barrier at the end) */
                    if (k0 < NS && ier == 0) {
                        SFOR(kk, 0, LU_NB) {
                            if (!PARTIAL || k0 + kk < NS) { L.piv[k0 + kk] = (uint8_t)pword[kk]; L.invp[k0 + kk] = mults[kk]; }
                        } SEND
                    }
                }
            }
            LUP_T(t_c)
            if (!first) {
                if (prev_round) { LU_UPD_MAIN(SQ) if (wave > o) { LU_UPD_SAME(SQ) } }
                else { LU_UPD_MAIN(S) if (wave > o) { LU_UPD_SAME(S) } }
            }
            if (wave == o && own_swaps != 0) {
                /* the owner's OTHER columns follow its panel's row exchanges only now: they had to receive panel p-1
                   (whose multipliers are indexed by the rows' places before these exchanges) first */
                SFOR(kk, 0, LU_NB) word[kk] = own_word[kk]; SEND
                LU_GATHER_MAP(S, k0)
                SFOR(cc, 0, pr * LU_NB) LU_GATHER_COL(S, a[cc]) SEND
                SFOR(cc, (pr + 1) * LU_NB, LU_NC) LU_GATHER_COL(S, a[cc]) SEND
            }
            LUP_T(t_d)
            LUP_ADD(0, t_b, t_c) LUP_ADD(1, t_a, t_b) LUP_ADD(2, t_c, t_d)
        }
    } SEND
    {   /* the row exchanges of the last panel */
        constexpr int PL = LU_NPANEL - 1, SL = LU_SLOT(LU_NPR - 1);
        double lc[LU_NB][RS];
        int word[LU_NB];
        lu_wait(L.pub, PL + 1);
        LU_READ(SL, PL)
        (void)lc;
        LU_SWAPS(SL, PL * LU_NB, PL & (SA_WAVES - 1))
    }
#undef LU_SWAPS
#undef LU_GATHER_COL
#undef LU_GATHER_MAP
#undef LU_READ
#undef LU_UPD_MAIN
#undef LU_UPD_SAME
#undef LU_UPD_GROUP
    LUP_T(t_out)
    if (ier == 0) {
        /* factors -> LDS for the triangular solves: full register slots unmasked, the partial one under one lane mask;
           a padding column (wave-uniform, last round only) is skipped as a whole */
        SFOR(r, 0, RS) {
            if ((r + 1) * 64 <= NS || r * 64 + lane < NS) {
                SFOR(cc, 0, LU_NC) {
                    const int j = LU_COL(cc);
                    if ((cc / LU_NB + 1) * SA_WAVES * LU_NB <= NS || j < NS) L.A[j * NS + r * 64 + lane] = a[cc][r];
                } SEND
            }
        } SEND
    }
    if (wave == 0 && lane == 0) (*L.nswaps) = nswaps;
    LUP_T(t_wr)
    sa_barrier();
    LUP_T(t_end)
    LUP_ADD(4, t_in, t_end) LUP_ADD(7, t_out, t_wr) LUP_ADD(8, t_wr, t_end)
#ifdef SA_WAVE_PROFILE
    if (wave == 0 && lane == 0) L.prof[3] += (int64_t)wall_clock64() - w_in;        /* 10 ns ticks over the same span */
#endif
#undef LU_COL
}
#else
static __device__ __forceinline__ LuLds lu_lds() { return LuLds{nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr}; }
static __device__ void setup_lu_regs(int, int, double, int, double *, LuLds) {}
static __device__ __forceinline__ void setup_lu_regs_body(int, int, double, int, double *, LuLds) {}
#endif

template <bool BWD>
DEV int dense_getrf(Cw<BWD> &m)
{
    PROF_T0
    if constexpr (SA_WAVES > 1) {
        if (m.li == 0) s_cmd = CMD_GETRF;
        sa_barrier();
    }
    const Grp g{m.lane, m.li, m.gbase, m.abase, m.kbase, 0};
    int ier;
    if constexpr (SA_WAVES == 1 && G < 64 && NS * RS <= LU_GROUP_REGS_MAX) ier = getrf_group_regs(g, m.inv_piv, m.nswaps);
    else ier = getrf_coop(g, m.inv_piv, m.nswaps);
    if constexpr (SA_WAVES > 1) sa_barrier();
    lds_sync();
    PROF_ADD(m, 3)
    return ier;
}

#if SA_WAVES > 1
/* wavefront 0's side of setup_lu_regs: publish the command, take part, collect pivots' reciprocals */
template <bool BWD>
DEV int setup_lu_workgroup(Cw<BWD> &m, double c, bool from_saved)
{
    PROF_T0
    if (m.li == 0) { s_cmd = CMD_GETRF; s_targ = c; s_flag = from_saved ? 1 : 0; }
    sa_barrier();
    setup_lu_regs(0, m.lane, c, from_saved ? 1 : 0, m.sj, lu_lds());
    const int ier = s_luier;
    m.nswaps = s_lunswaps;
    SFOR(r, 0, RS) { const int i = r * 64 + m.lane; m.inv_piv[r] = (i < NS) ? s_invp[i < NS ? i : 0] : 0.0; } SEND
    sa_barrier();                /* pairs with the barrier that ends every pass of worker_loop */
    lds_sync();
    PROF_ADD(m, 3)
    return ier;
}
#endif

/* component k (wave-uniform k) of a lane-distributed vector */
DEV double bcast_vec(const double (&b)[RS], int k, int gbase)
{
    double v = b[0];
    SFOR(r, 1, RS) v = ((k / G) == r) ? b[r] : v; SEND
    if constexpr (G == 64) return readlane_d(v, k & 63);        /* k is wave-uniform */
    else return shfl_d(v, gbase + (k & (G - 1)));               /* k is uniform within the group only */
}

/* Triangular solves for the whole-wavefront mapping (G = 64): the chain through b is inherently serial
   (broadcast b_k, one FMA per owned row) and -- for a lone wavefront -- paid per INSTRUCTION (four cycles each,
   profiles/r04_ubench_issue.txt), so everything else is taken out of it: the loops are split by the register slot that
   holds b_k (no slot selects), the matrix columns come from LDS a block of GETRS_BLOCK columns ahead (double-buffered),
   and there are NO ROW MASKS (round 4): the finished component of a step is filed in a second vector with one
   v_writelane per half, after which the FMA may run over every row of the slot -- the rows it must not touch (those
   already solved, whose matrix entries belong to the other factor) are dead values in b by then.  Per step: two
   v_readlane, two v_writelane, one FMA per slot (before: two more v_readlane for a spilled lane mask and two
   v_cndmask).  Same operations on the same values for every component that is ever read. */
#ifndef GETRS_BLOCK
#define GETRS_BLOCK 4
#endif
template <int LANE>
DEV double writelane_d(double old, double v)                   /* old with lane LANE replaced by the (wave-uniform) v */
{
    static_assert(LANE >= 0 && LANE < 64, "lane of a wavefront");
    const uint64_t u = __builtin_bit_cast(uint64_t, v);
    uint64_t o = __builtin_bit_cast(uint64_t, old);
    uint32_t lo = (uint32_t)o, hi = (uint32_t)(o >> 32);
    /* (this clang has no __builtin_amdgcn_writelane; the lane select is an inline constant: one scalar operand only) */
    asm("v_writelane_b32 %0, %1, %2" : "+v"(lo) : "s"((uint32_t)u), "n"(LANE));
    asm("v_writelane_b32 %0, %1, %2" : "+v"(hi) : "s"((uint32_t)(u >> 32)), "n"(LANE));
    return __builtin_bit_cast(double, ((uint64_t)hi << 32) | (uint64_t)lo);
}
template <bool BWD>
DEV void dense_getrs64(Cw<BWD> &m, double (&b)[RS])
{
    const int lane = m.lane;
    const double *A = s_A + m.abase;
    const double (&inv_piv)[RS] = m.inv_piv;
    double y[RS];                                   /* the solved components, filed as they become final */
    SFOR(r, 0, RS) y[r] = b[r]; SEND
    /* forward substitution with the unit lower factor */
    SFOR(sk, 0, RS) {
        constexpr int k_lo = sk * 64;
        constexpr int k_hi = (NS - 1 < k_lo + 64) ? NS - 1 : k_lo + 64;
        if constexpr (k_lo < k_hi) {
            double nxt[GETRS_BLOCK][RS], cur[GETRS_BLOCK][RS];
            SFOR(d, 0, GETRS_BLOCK) { SFOR(r, sk, RS) nxt[d][r] = A[(k_lo + d < NS ? k_lo + d : 0) * NS + r * 64 + lane]; SEND } SEND
            /* the steps are unrolled (k is a compile-time index: immediate lane selects, no loop or bounds
               bookkeeping, no register copies between the prefetch buffers) */
            SFOR(kb, 0, (k_hi - k_lo + GETRS_BLOCK - 1) / GETRS_BLOCK) {
                constexpr int k0 = k_lo + kb * GETRS_BLOCK;
                __builtin_amdgcn_sched_barrier(0);      /* keep the scheduler from pulling later blocks' loads up */
                SFOR(d, 0, GETRS_BLOCK) { SFOR(r, sk, RS) cur[d][r] = nxt[d][r]; SEND } SEND
                SFOR(d, 0, GETRS_BLOCK) {
                    constexpr int kn = k0 + GETRS_BLOCK + d;
                    if constexpr (kn < k_hi) { SFOR(r, sk, RS) nxt[d][r] = A[kn * NS + r * 64 + lane]; SEND }
                } SEND
                SFOR(d, 0, GETRS_BLOCK) {
                    constexpr int k = k0 + d;
                    if constexpr (k < k_hi) {
                        const double bk = readlane_d(b[sk], k - k_lo);
                        y[sk] = writelane_d<k - k_lo>(y[sk], bk);
                        SFOR(r, sk, RS) b[r] = FMA(-cur[d][r], bk, b[r]); SEND
                    }
                } SEND
            } SEND
        }
        /* the rows of this slot that no step of it finalised (the last row of the system; a slot the loop above did
           not enter): they are final now -- rows beyond the steps only ever received their own updates */
        {
            constexpr int done_to = (k_lo < k_hi) ? k_hi - k_lo : 0;       /* lanes [0, done_to) are filed */
            y[sk] = (lane >= done_to) ? b[sk] : y[sk];
        }
    } SEND
    SFOR(r, 0, RS) b[r] = y[r]; SEND
    /* back substitution with the upper factor (reciprocal pivots) */
    SFOR_DOWN(sk, RS - 1, 0) {
        constexpr int k_lo = sk * 64 > 1 ? sk * 64 : 1;                 /* k = NS-1 ... 1 */
        constexpr int k_hi = (NS - 1 < sk * 64 + 63) ? NS - 1 : sk * 64 + 63;
        if constexpr (k_lo <= k_hi) {
            double nxt[GETRS_BLOCK][RS], cur[GETRS_BLOCK][RS];
            SFOR(d, 0, GETRS_BLOCK) { SFOR(r, 0, sk + 1) nxt[d][r] = A[(k_hi - d > 0 ? k_hi - d : 0) * NS + r * 64 + lane]; SEND } SEND
            SFOR(kb, 0, (k_hi - k_lo + GETRS_BLOCK) / GETRS_BLOCK) {
                constexpr int k0 = k_hi - kb * GETRS_BLOCK;
                __builtin_amdgcn_sched_barrier(0);
                SFOR(d, 0, GETRS_BLOCK) { SFOR(r, 0, sk + 1) cur[d][r] = nxt[d][r]; SEND } SEND
                SFOR(d, 0, GETRS_BLOCK) {
                    constexpr int kn = k0 - GETRS_BLOCK - d;
                    if constexpr (kn >= k_lo) { SFOR(r, 0, sk + 1) nxt[d][r] = A[kn * NS + r * 64 + lane]; SEND }
                } SEND
                SFOR(d, 0, GETRS_BLOCK) {
                    constexpr int k = k0 - d;
                    if constexpr (k >= k_lo) {
                        constexpr int kl = k - sk * 64;
                        const double scaled = b[sk] * inv_piv[sk];
                        const double bk = readlane_d(scaled, kl);
                        y[sk] = writelane_d<kl>(y[sk], bk);
                        SFOR(r, 0, sk + 1) b[r] = FMA(-cur[d][r], bk, b[r]); SEND
                    }
                } SEND
            } SEND
        }
    } SEND
    /* component 0 (never a step of the loops above: k runs down to 1) */
    {
        const double scaled = b[0] * inv_piv[0];
        y[0] = writelane_d<0>(y[0], readlane_d(scaled, 0));
    }
    SFOR(r, 0, RS) b[r] = (r * 64 + lane >= NS) ? 0.0 : y[r]; SEND
}

/* ---- triangular solves of an 8-lane group, unrolled (small systems: config 4) ----
 * The chain through b is serial: broadcast b_k, one FMA per owned row, next k.  With k a compile-time index the
 * source lane of the broadcast (k mod 8 of every group) is static, so it is two DPP moves per 32-bit half -- a
 * quad-permute that fills the source quad, a row_half_mirror under a bank mask that copies it into the other quad
 * of the group -- ~30 cycles of VALU latency in the chain instead of the ~150 of a ds_bpermute round trip.  The
 * row masks (i > k, i < k) are folded into the matrix entries (zero where the row takes no part), matrix columns come
 * from LDS a block of GETRS_BLOCK8 columns ahead.  Same operations on the same values as the generic loop. */
#define GETRS_BLOCK8 4
template <int C>
static __device__ __forceinline__ double sa_bcast8(double v)
{
    static_assert(C >= 0 && C < 8, "lane of an 8-lane group");
    const uint64_t u = __builtin_bit_cast(uint64_t, v);
    int lo = (int)(uint32_t)u, hi = (int)(uint32_t)(u >> 32);
    constexpr int c4 = C & 3, qp = c4 | (c4 << 2) | (c4 << 4) | (c4 << 6);
    constexpr int bank = (C < 4) ? 0xA : 0x5;           /* banks (quads of a 16-lane row) to overwrite */
    lo = __builtin_amdgcn_update_dpp(lo, lo, qp, 0xF, 0xF, false);
    hi = __builtin_amdgcn_update_dpp(hi, hi, qp, 0xF, 0xF, false);
    lo = __builtin_amdgcn_update_dpp(lo, lo, 0x141, 0xF, bank, false);
    hi = __builtin_amdgcn_update_dpp(hi, hi, 0x141, 0xF, bank, false);
    return __builtin_bit_cast(double, ((uint64_t)(uint32_t)hi << 32) | (uint64_t)(uint32_t)lo);
}

template <bool BWD>
DEV void dense_getrs_group8(Cw<BWD> &m, double (&b)[RS])
{
    const Grp g{m.lane, m.li, m.gbase, m.abase, m.kbase, 0};
    /* forward substitution with the unit lower factor: columns 0 .. NS-2 */
    {
        double nxt[GETRS_BLOCK8][RS], cur[GETRS_BLOCK8][RS];
        SFOR(d, 0, GETRS_BLOCK8) {
            SFOR(r, 0, RS) { const int i = r * 8 + g.li; nxt[d][r] = (d < NS - 1 && i > d && i < NS) ? AL(i < NS ? i : 0, d < NS ? d : 0) : 0.0; } SEND
        } SEND
        SFOR(kb, 0, (NS - 1 + GETRS_BLOCK8 - 1) / GETRS_BLOCK8) {
            constexpr int k0 = kb * GETRS_BLOCK8;
            __builtin_amdgcn_sched_barrier(0);
            SFOR(d, 0, GETRS_BLOCK8) { SFOR(r, 0, RS) cur[d][r] = nxt[d][r]; SEND } SEND
            SFOR(d, 0, GETRS_BLOCK8) {
                constexpr int kn = k0 + GETRS_BLOCK8 + d;
                if constexpr (kn < NS - 1) {
                    SFOR(r, 0, RS) { const int i = r * 8 + g.li; nxt[d][r] = (i > kn && i < NS) ? AL(i < NS ? i : 0, kn) : 0.0; } SEND
                }
            } SEND
            SFOR(d, 0, GETRS_BLOCK8) {
                constexpr int k = k0 + d;
                if constexpr (k < NS - 1) {
                    const double bk = sa_bcast8<(k & 7)>(b[k / 8]);
                    SFOR(r, k / 8, RS) b[r] = FMA(-cur[d][r], bk, b[r]); SEND
                }
            } SEND
        } SEND
    }
    /* back substitution with the upper factor (reciprocal pivots): columns NS-1 .. 1 */
    {
        double nxt[GETRS_BLOCK8][RS], cur[GETRS_BLOCK8][RS];
        SFOR(d, 0, GETRS_BLOCK8) {
            SFOR(r, 0, RS) { const int i = r * 8 + g.li; nxt[d][r] = (NS - 1 - d > 0 && i < NS - 1 - d) ? AL(i, NS - 1 - d > 0 ? NS - 1 - d : 0) : 0.0; } SEND
        } SEND
        SFOR(kb, 0, (NS - 1 + GETRS_BLOCK8 - 1) / GETRS_BLOCK8) {
            constexpr int k0 = NS - 1 - kb * GETRS_BLOCK8;
            __builtin_amdgcn_sched_barrier(0);
            SFOR(d, 0, GETRS_BLOCK8) { SFOR(r, 0, RS) cur[d][r] = nxt[d][r]; SEND } SEND
            SFOR(d, 0, GETRS_BLOCK8) {
                constexpr int kn = k0 - GETRS_BLOCK8 - d;
                if constexpr (kn > 0) {
                    SFOR(r, 0, RS) { const int i = r * 8 + g.li; nxt[d][r] = (i < kn) ? AL(i, kn) : 0.0; } SEND
                }
            } SEND
            SFOR(d, 0, GETRS_BLOCK8) {
                constexpr int k = k0 - d;
                if constexpr (k > 0) {
                    constexpr int sk = k / 8;
                    const double scaled = b[sk] * m.inv_piv[sk];
                    b[sk] = (g.li == (k & 7)) ? scaled : b[sk];
                    const double bk = sa_bcast8<(k & 7)>(b[sk]);
                    SFOR(r, 0, sk + 1) b[r] = FMA(-cur[d][r], bk, b[r]); SEND
                }
            } SEND
        } SEND
    }
    if (m.li == 0) b[0] *= m.inv_piv[0];
}

#if SA_LEAN
/* ---- lean lane groups: LU and triangular solves on REGISTER-resident factors (m.lu) -------------------------------
 * Lane li of a group owns rows li, li + G, ... of every column (NS*RS doubles).  I - gamma*J is close to diagonally
 * dominant: partial pivoting all but never exchanges rows, so the factorisation runs SPECULATIVELY without exchanges --
 * every row stays in its home lane and slot, the elimination index k is a compile-time constant, and every broadcast
 * (pivot, pivot-row entry, b_k of the solves) is a static DPP pattern: quad-permute for four lanes per instance, two
 * DPP moves for eight (sa_bcast8) -- no ds_bpermute, no LDS, no ballot per step.  Each lane records whether one of
 * its rows ever beat the pivot (denseGETRF's strict '>' test); a group where that happened -- and only such a group --
 * is factorised again by getrf_coop (LDS, explicit exchanges, pivots to s_piv) in the one-matrix scratch s_A, one
 * group at a time, and reloads its factors from there.  Same operations on the same values as denseGETRF / denseGETRS
 * in both cases (test_row_exchanges_in_the_dense_lu drives the fall-back). */
template <int C>
static __device__ __forceinline__ double sa_bcast_grp(double v)
{
    static_assert(C >= 0 && C < G, "lane of the group");
    if constexpr (G == 8) return sa_bcast8<C>(v);
    else {
        if constexpr (G == 1) return v;
        static_assert(G == 4 || G == 2 || G == 1, "static group broadcasts: 1, 2, 4 or 8 lanes per instance");
        constexpr int qp = (G == 4) ? (C | (C << 2) | (C << 4) | (C << 6)) : (C | (C << 2) | ((C + 2) << 4) | ((C + 2) << 6));
        const uint64_t u = __builtin_bit_cast(uint64_t, v);
        int lo = (int)(uint32_t)u, hi = (int)(uint32_t)(u >> 32);
        lo = __builtin_amdgcn_update_dpp(lo, lo, qp, 0xF, 0xF, false);
        hi = __builtin_amdgcn_update_dpp(hi, hi, qp, 0xF, 0xF, false);
        return __builtin_bit_cast(double, ((uint64_t)(uint32_t)hi << 32) | (uint64_t)(uint32_t)lo);
    }
}
/* row r*G + li is a real row (compile-time true for slots without padding) */
#define LEAN_REAL(r, li) ((((r) + 1) * G <= NS) ? true : ((r) * G + (li) < NS))

template <bool BWD>
DEV int getrf_lean(Cw<BWD> &m, bool &beaten)
{
    int ier = 0;
    beaten = false;
    SFOR(k, 0, NS) {
        constexpr int sk = k / G, lk = k % G;
        const double akk = sa_bcast_grp<lk>(m.lu[k][sk]);
        const double best = fabs(akk);
        bool below[RS];
        SFOR(r, sk, RS) {
            below[r] = (r > sk) ? LEAN_REAL(r, m.li) : (m.li > lk && LEAN_REAL(r, m.li));
            beaten = beaten || (below[r] && fabs(m.lu[k][r]) > best);
        } SEND
        ier = (ier == 0 && akk == 0.0) ? k + 1 : ier;       /* (a zero pivot with a non-zero row below it: beaten) */
        const double mult = 1.0 / akk;
        m.inv_piv[sk] = (m.li == lk) ? mult : m.inv_piv[sk];
        double lc[RS];
        SFOR(r, sk, RS) {
            lc[r] = below[r] ? m.lu[k][r] * mult : 0.0;
            m.lu[k][r] = below[r] ? lc[r] : m.lu[k][r];
        } SEND
        SFOR(j, k + 1, NS) {
            const double akj = sa_bcast_grp<lk>(m.lu[j][sk]);
            SFOR(r, sk, RS) m.lu[j][r] = FMA(-akj, lc[r], m.lu[j][r]); SEND
        } SEND
    } SEND
    return ier;
}

/* M = I + c*J (c = -gamma) from the saved Jacobian in the workspace, straight into the factor registers.
   (Measured and not kept: a second, lane-ordered copy of the saved Jacobian -- [column][slot][lane], one coalesced
   512-byte load per entry instead of 16 scattered 32-byte pieces -- bit-exact and 63 % SLOWER, SEIR backward 51.9 ->
   84.8 ms: the copy adds 4 MB of hot data per XCD next to the 4 MB of natural-layout Jacobians and 3.7 MB of scratch
   that already compete for the 4 MB L2, and the allocator answered the change with 352 instead of 208 spill slots.) */
template <bool BWD>
DEV void lean_load_matrix(Cw<BWD> &m, double c)
{
    const gdouble *sjg = (const gdouble *)m.sj;
    SFOR(j, 0, NS) {
        SFOR(r, 0, RS) {
            const int row = r * G + m.li;
            const double v = sjg[j * NS + (LEAN_REAL(r, m.li) ? row : 0)];
            const double w = (row == j) ? FMA(c, v, 1.0) : v * c;
            m.lu[j][r] = LEAN_REAL(r, m.li) ? w : 0.0;
        } SEND
    } SEND
}

template <bool BWD>
DEV int lean_factor(Cw<BWD> &m, double c)
{
    bool beaten;
    m.nswaps = 0;
    lean_load_matrix(m, c);
    int ier = getrf_lean(m, beaten);
    const uint64_t need = __builtin_amdgcn_ballot_w64(beaten);
    if (need != 0) {                                    /* rare: some group needs a row exchange */
        for (int g = 0; g < KPW; g++) {
            if (((need >> (g * G)) & GMASK) == 0) continue;
            if (m.lane / G == g) {
                const gdouble *sjg = (const gdouble *)m.sj;
                lds_sync();
                for (int idx = m.li; idx < NS * NS; idx += G) {
                    const double v = sjg[idx];
                    s_A[idx] = (idx % NS == idx / NS) ? FMA(c, v, 1.0) : v * c;
                }
                lds_sync();
                const Grp gg{m.lane, m.li, m.gbase, 0, m.kbase, 0};
                ier = getrf_coop(gg, m.inv_piv, m.nswaps);
                lds_sync();
                SFOR(j, 0, NS) {
                    SFOR(r, 0, RS) {
                        const int row = r * G + m.li;
                        m.lu[j][r] = LEAN_REAL(r, m.li) ? s_A[j * NS + (LEAN_REAL(r, m.li) ? row : 0)] : 0.0;
                    } SEND
                } SEND
                lds_sync();
            }
        }
    }
    return ier;
}

/* denseGETRS on the register factors (after the row permutation of b, done by the caller through s_piv) */
template <bool BWD>
DEV void getrs_lean(Cw<BWD> &m, double (&b)[RS])
{
    SFOR(k, 0, NS - 1) {                                /* unit lower factor */
        constexpr int sk = k / G, lk = k % G;
        const double bk = sa_bcast_grp<lk>(b[sk]);
        SFOR(r, sk, RS) {
            const double l = (r > sk) ? m.lu[k][r] : ((m.li > lk) ? m.lu[k][r] : 0.0);
            b[r] = FMA(-l, bk, b[r]);
        } SEND
    } SEND
    SFOR_DOWN(k, NS - 1, 1) {                           /* upper factor, reciprocal pivots */
        constexpr int sk = k / G, lk = k % G;
        const double scaled = b[sk] * m.inv_piv[sk];
        b[sk] = (m.li == lk) ? scaled : b[sk];
        const double bk = sa_bcast_grp<lk>(b[sk]);
        SFOR(r, 0, sk + 1) {
            const double u = (r < sk) ? m.lu[k][r] : ((m.li < lk) ? m.lu[k][r] : 0.0);
            b[r] = FMA(-u, bk, b[r]);
        } SEND
    } SEND
    if (m.li == 0) b[0] *= m.inv_piv[0];
    SFOR(r, 0, RS) { if (!LEAN_REAL(r, m.li)) b[r] = 0.0; } SEND
}
#endif

template <bool BWD>
DEV void dense_getrs(Cw<BWD> &m, double (&b)[RS])
{
    PROF_T0
    const Grp g{m.lane, m.li, m.gbase, m.abase, m.kbase, 0};
    if (m.nswaps != 0) {               /* row permutation through the LDS scratch vector */
        lds_sync();
        SFOR(r, 0, RS) { if (IDX(m, r) < NS) s_lam[m.vbase + IDX(m, r)] = b[r]; } SEND
        lds_sync();
        for (int k = 0; k < NS; k++) {
            const int pk = s_piv[m.kbase + k];
            if (pk != k) {
                const double bk = s_lam[m.vbase + k], bp = s_lam[m.vbase + pk];
                lds_sync();
                if (m.li == 0) { s_lam[m.vbase + k] = bp; s_lam[m.vbase + pk] = bk; }
                lds_sync();
            }
        }
        SFOR(r, 0, RS) { if (IDX(m, r) < NS) b[r] = s_lam[m.vbase + IDX(m, r)]; } SEND
        lds_sync();
    }
    if constexpr (G == 64) {
        dense_getrs64(m, b);
        PROF_ADD(m, 4)
        return;
    }
#if SA_LEAN
    getrs_lean(m, b);
    PROF_ADD(m, 4)
    return;
#endif
    if constexpr (G == 8 && SA_WAVES == 1 && NS <= 32) {
        dense_getrs_group8(m, b);
        PROF_ADD(m, 4)
        return;
    }
    /* The chain through b is inherently serial (one broadcast + one FMA per step); the matrix column of the
       NEXT step does not depend on it, so it is fetched from LDS one step ahead (GETRS_DEPTH columns in
       flight) instead of inside the dependent chain. */
    {
        double col[GETRS_DEPTH][RS];
        SFOR(d, 0, GETRS_DEPTH) {
            SFOR(r, 0, RS) { const int i = IDX(m, r); col[d][r] = (d < NS - 1 && i > d && i < NS) ? AL(i, d) : 0.0; } SEND
        } SEND
        for (int k0 = 0; k0 < NS - 1; k0 += GETRS_DEPTH) {
            SFOR(d, 0, GETRS_DEPTH) {
                const int k = k0 + d;
                if (k < NS - 1) {
                    double cur[RS];
                    SFOR(r, 0, RS) cur[r] = col[d][r]; SEND
                    const int kn = k + GETRS_DEPTH;          /* refill this slot with the column GETRS_DEPTH ahead */
                    SFOR(r, 0, RS) { const int i = IDX(m, r); col[d][r] = (kn < NS - 1 && i > kn && i < NS) ? AL(i, kn) : 0.0; } SEND
                    const double bk = bcast_vec(b, k, m.gbase);
                    SFOR(r, 0, RS) { const int i = IDX(m, r); if (i > k && i < NS) b[r] = FMA(-cur[r], bk, b[r]); } SEND
                }
            } SEND
        }
        SFOR(d, 0, GETRS_DEPTH) {
            const int k = NS - 1 - d;
            SFOR(r, 0, RS) { const int i = IDX(m, r); col[d][r] = (k > 0 && i < k) ? AL(i, k) : 0.0; } SEND
        } SEND
        for (int k0 = NS - 1; k0 > 0; k0 -= GETRS_DEPTH) {
            SFOR(d, 0, GETRS_DEPTH) {
                const int k = k0 - d;
                if (k > 0) {
                    double cur[RS];
                    SFOR(r, 0, RS) cur[r] = col[d][r]; SEND
                    const int kn = k - GETRS_DEPTH;
                    SFOR(r, 0, RS) { const int i = IDX(m, r); col[d][r] = (kn > 0 && i < kn) ? AL(i, kn) : 0.0; } SEND
                    SFOR(r, 0, RS) { if (IDX(m, r) == k) b[r] *= m.inv_piv[r]; } SEND
                    const double bk = bcast_vec(b, k, m.gbase);
                    SFOR(r, 0, RS) { const int i = IDX(m, r); if (i < k) b[r] = FMA(-cur[r], bk, b[r]); } SEND
                }
            } SEND
        }
    }
    if (m.li == 0) b[0] *= m.inv_piv[0];
    PROF_ADD(m, 4)
}


#ifdef SA_SENS
/* ---- forward sensitivities in the lean lane groups (Solver(sens_mode=...), reference solver.py:360-392, 483-527;
 * sensitivity right-hand side symode/problem.py:557-583) -----------------------------------------------------------
 * Same corrector as the register kernel's -DSA_SENS build / the oracle (simultaneous: the sensitivity systems ride in
 * the state's Newton iteration; staggered: their own iteration after the state passed), but the NQ x 13 sensitivity
 * vectors do not fit any on-chip storage at n = 16, p = 8 (416 doubles per lane): they live in the workspace,
 * [vector][parameter][slot][lane] (a wavefront's 64 lanes touch 64 consecutive doubles), and every operation streams
 * them through registers.  The right-hand side J(t,y) s_i + df/dp_i takes J and df/dp from the generated callbacks
 * (written to the workspace by all lanes of the group), each lane then accumulates its rows for all parameters with
 * the entries of s_i broadcast across the group by static DPP moves -- the association of the oracle's cv_fS. */
static_assert(SA_LEAN, "the sensitivity corrector of bdf_wave.hip exists in the lean lane-group builds (n <= 21); larger: bdf_mem.hip");
#define SENS_ON(m) (!BWD && (m).sensi)
#define SV(m, v, is, r) (m).sws[(int64_t)(((v) * NQ + (is)) * RS + (r)) * 64]
/* the loop over the parameters stays a LOOP: unrolled (what -O3 does with a trip count of 8) the loads of all
   parameters' vectors are hoisted in front of the arithmetic and the kernel spills -- SEIR: 1 585 spill slots and 4 KB of
   scratch per lane unrolled, 592 / 1 KB as a loop (profiles/r06_sens_nounroll.txt; -DSA_SENS_UNROLL: the round-5 form) */
#ifdef SA_SENS_UNROLL
#define SLOOP_BEGIN(is) for (int is = 0; is < NQ; is++) {
#else
#define SLOOP_BEGIN(is) _Pragma("nounroll") for (int is = 0; is < NQ; is++) {
#endif
#define SLOOP_END }

/* out[is] = J ys[is] + dp[is] for the rows of this lane; J, dp: workspace copies the callbacks just wrote */
#define SENS_RHS_ATTR __attribute__((noinline))
static __device__ SENS_RHS_ATTR int sens_rhs_rows(double *sws, const gdouble *js, const gdouble *dp, int li,
                                                              int v_in, int v_out)
{
    double ys[NQ][RS], acc[NQ][RS];
    SFOR(is, 0, NQ) { SFOR(r, 0, RS) ys[is][r] = sws[(int64_t)((v_in * NQ + is) * RS + r) * 64]; SEND } SEND
    SFOR(j, 0, NS) {
        double jrow[RS];
        SFOR(r, 0, RS) jrow[r] = js[j * NS + (LEAN_REAL(r, li) ? r * G + li : 0)]; SEND
        SFOR(is, 0, NQ) {
            const double yj = sa_bcast_grp<(j % G)>(ys[is][j / G]);
            SFOR(r, 0, RS) acc[is][r] = (j == 0) ? jrow[r] * yj : FMA(jrow[r], yj, acc[is][r]); SEND
        } SEND
    } SEND
    bool bad = false;
    SFOR(is, 0, NQ) {
        SFOR(r, 0, RS) {
            const double a = acc[is][r] + dp[is * NS + (LEAN_REAL(r, li) ? r * G + li : 0)];
            sws[(int64_t)((v_out * NQ + is) * RS + r) * 64] = LEAN_REAL(r, li) ? a : 0.0;
            bad = bad || (LEAN_REAL(r, li) && !(a * 0.0 == 0.0));
        } SEND
    } SEND
    return bad ? 1 : 0;
}

template <int v_in, int v_out, bool BWD>
DEV int cv_fS(Cw<BWD> &m, double t, const double (&y)[RS])
{
    m.nfSe++;
    stage_inputs(m, y);
    gdouble *js = (gdouble *)(m.sj - WS_SJ + WS_JS), *dp = (gdouble *)(m.sj - WS_SJ + WS_DP);
    int rc = sa_jac(t, nullptr, nullptr, m.pr, GMatOut{js});
    if (rc != 0) return rc;
    rc = sa_dydp(t, nullptr, nullptr, m.pr, GMatOut{dp});
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    const int bad = sens_rhs_rows(m.sws, js, dp, m.li, v_in, v_out);
    const uint64_t any = __builtin_amdgcn_ballot_w64(bad != 0);
    return (rc != 0 || ((any >> m.gbase) & GMASK) != 0) ? 1 : 0;
}

#endif

/* ---- linear solver interface ---- */
#define COPY_BATCH 8
template <bool BWD>
DEV int cv_lsetup(Cw<BWD> &m, int convfail)
{
    double dgamma = fabs((m.gamma / m.gammap) - 1.0);
    int jbad = (m.nst == 0) || (m.nst > m.nstlj + MSBJ) ||
               ((convfail == CV_FAIL_BAD_J) && (dgamma < CVLS_DGMAX)) ||
               (convfail == CV_FAIL_OTHER);
    int jret = 0;
    const double c = -m.gamma;
    lds_sync();
#if SA_LEAN
    {   /* J (fresh: the callback wrote it to the workspace; else the saved copy) -> I - gamma*J -> LU, in registers */
        if (!jbad) m.jcur = 0;
        else {
            m.nje++;
            m.nstlj = m.nst;
            m.jcur = 1;
            jret = cv_jac(m, m.tn, m.y);
            /* the group's lanes wrote the entries; every lane now reads its rows */
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
        }
        if (jret < 0) return -1;
        if (jret > 0) return 1;
        PROF_T0
        const int ier = lean_factor(m, c);
        PROF_ADD(m, 3)
        return ier > 0 ? 1 : 0;
    }
#endif
#if SA_WAVES > 1
    {   /* whole workgroup: J (saved copy, or fresh from the callback via LDS) -> I - gamma*J -> LU, in registers */
        if (!jbad) m.jcur = 0;
        else {
            m.nje++;
            m.nstlj = m.nst;
            m.jcur = 1;
            jret = cv_jac(m, m.tn, m.y);
        }
        if (jret < 0) return -1;
        if (jret > 0) return 1;
        const int ier = setup_lu_workgroup(m, c, !jbad);
        return ier > 0 ? 1 : 0;
    }
#endif
    if (!jbad) {
        PROF_T0
        m.jcur = 0;
        /* A = I - gamma * savedJ, streamed from the workspace (COPY_BATCH loads in flight per lane) */
        int base = 0;
        for (; base + COPY_BATCH * G <= NS * NS; base += COPY_BATCH * G) {
            double v[COPY_BATCH];
            SFOR(u, 0, COPY_BATCH) v[u] = m.sj[base + u * G + m.li]; SEND
            SFOR(u, 0, COPY_BATCH) {
                const int idx = base + u * G + m.li;
                s_A[m.abase + idx] = (idx % NS == idx / NS) ? FMA(c, v[u], 1.0) : v[u] * c;
            } SEND
        }
        for (int idx = base + m.li; idx < NS * NS; idx += G) {
            const double v = m.sj[idx];
            s_A[m.abase + idx] = (idx % NS == idx / NS) ? FMA(c, v, 1.0) : v * c;
        }
        PROF_ADD(m, 5)
    } else {
        m.nje++;
        m.nstlj = m.nst;
        m.jcur = 1;
        jret = cv_jac(m, m.tn, m.y);
        if (jret == 0) {
            for (int idx = m.li; idx < NS * NS; idx += G) {
                const double v = s_A[m.abase + idx];
                m.sj[idx] = v;
                s_A[m.abase + idx] = (idx % NS == idx / NS) ? FMA(c, v, 1.0) : v * c;
            }
        }
    }
    lds_sync();
    if (jret < 0) return -1;
    if (jret > 0) return 1;
    int ier = dense_getrf(m);
    return ier > 0 ? 1 : 0;
}


#if SA_COLD_PARK
template <bool BWD>
DEV void cold_store(const Cw<BWD> &m)
{
    double *c = s_cold + m.lane;
    SFOR(j, 2, (QMAX) + 1) { SFOR(r, 0, RS) c[((j - 2) * RS + r) * 64] = m.zn[j][r]; SEND } SEND
    SFOR(r, 0, RS) c[(4 * RS + r) * 64] = m.zsave[r]; SEND
    if (BWD) {
        SFOR(j, 0, (QMAX) + 1) { SFOR(r, 0, RQ) c[(5 * RS + j * RQ + r) * 64] = m.znQ[j][r]; SEND } SEND
        SFOR(r, 0, RQ) c[(5 * RS + 6 * RQ + r) * 64] = m.zsaveQ[r]; SEND
    }
#if !defined(SA_NO_CTL_PARK)
    if (m.li == 0) {
        double *u = s_ctl + (m.lane / G) * W_NCTL;
        SFOR(i, 0, 6) u[i] = m.l[i]; SEND
        SFOR(i, 1, 6) u[5 + i] = m.tau[i]; SEND
        u[11] = m.tq[1]; u[12] = m.tq[3]; u[13] = m.tq[5];
    }
    lds_sync();         /* lane 0 wrote what the other lanes of the group read back: the fence keeps the compiler from
                           moving their loads above the (for them absent) store */
#endif
}
template <bool BWD>
DEV void cold_load(Cw<BWD> &m)
{
    const double *c = s_cold + m.lane;
    SFOR(j, 2, (QMAX) + 1) { SFOR(r, 0, RS) m.zn[j][r] = c[((j - 2) * RS + r) * 64]; SEND } SEND
    SFOR(r, 0, RS) m.zsave[r] = c[(4 * RS + r) * 64]; SEND
    if (BWD) {
        SFOR(j, 0, (QMAX) + 1) { SFOR(r, 0, RQ) m.znQ[j][r] = c[(5 * RS + j * RQ + r) * 64]; SEND } SEND
        SFOR(r, 0, RQ) m.zsaveQ[r] = c[(5 * RS + 6 * RQ + r) * 64]; SEND
    }
#if !defined(SA_NO_CTL_PARK)
    {
        lds_sync();
        const double *u = s_ctl + (m.lane / G) * W_NCTL;
        SFOR(i, 0, 6) m.l[i] = u[i]; SEND
        SFOR(i, 1, 6) m.tau[i] = u[5 + i]; SEND
        m.tq[1] = u[11]; m.tq[3] = u[12]; m.tq[5] = u[13];
    }
#endif
}
#define COLD_STORE(m) cold_store(m)
#define COLD_LOAD(m) cold_load(m)
#else
#define COLD_STORE(m)
#define COLD_LOAD(m)
#endif

#define SA_POLY_CM(BWD) 1                   /* pow coefficients from constant memory (sa_common.h): SEIR +7 %, network100 +1 %, network24 +-0 */
#define SA_STATE Cw
#include "bdf_core.h"

template <bool BWD>
DEV void setup_common(Cw<BWD> &m, const double *ps, const double *pr, int rem_stride, int inst, double *ws)
{
    m.lane = lane_id();
    m.li = m.lane & (G - 1);
    m.gbase = m.lane & ~(G - 1);
    {
        const int grp = m.lane / G;
        m.abase = SA_LEAN ? 0 : grp * NS * NS; m.vbase = grp * W_NSP; m.pbase = grp * W_NQP; m.kbase = grp * W_PIV;
        m.obase = grp * W_NOUTP;
    }
    m.pr = pr + (int64_t)inst * rem_stride;
    m.sj = ws_inst(ws, inst) + WS_SJ;
    m.obuf = ws_inst(ws, inst) + WS_OUT;
#ifdef SA_SENS
    m.sws = ws + (int64_t)(inst / KPW * KPW) * WS_DOUBLES + (int64_t)KPW * WS_SMALL + m.lane;
    m.sensi = 0; m.ism = 0; m.pbar = nullptr;
#endif
    for (int j = m.li; j < NQ; j += G) s_ps[m.pbase + j] = ps[(int64_t)inst * NQ + j];
    m.nswaps = 0;
    SFOR(r, 0, RS) { m.inv_piv[r] = 0.0; m.ytmp[r] = 0.0; m.ewt[r] = 0.0; } SEND
    SFOR(r, 0, RQ) m.ewtQ[r] = 0.0; SEND
#if SA_TAB_LDS
    for (int f = m.li; f < W_TREC; f += G) s_tab[(m.lane / G) * W_TRECP + f] = (f == 1) ? 1.0 : 0.0;
#else
    SFOR(f, 0, 8) m.tab_hdr[f] = (f == 1) ? 1.0 : 0.0; SEND
    SFOR(j, 0, (QMAX) + 1) { SFOR(r, 0, RS) m.tabY[j][r] = 0.0; SEND } SEND
#endif
#if SA_LEAN
    SFOR(j, 0, NS) { SFOR(r, 0, RS) m.lu[j][r] = 0.0; SEND } SEND
#endif
#ifdef SA_WAVE_PROFILE
    SFOR(i, 0, 8) m.prof[i] = 0; SEND
    m.prof[7] = -(int64_t)wall_clock64();
#endif
    lds_sync();
}

#ifdef SA_HERMITE
/* CV_HERMITE data point: {t, y, y'} in the slots rec[2], rec[8 + i], rec[8 + n + i] of a record */
DEV void store_hermite(double *rec, int li, double t, const double (&y)[RS], const double (&yd)[RS])
{
    if (li == 0) { rec[0] = 0.0; rec[1] = 1.0; rec[2] = t; }
    SFOR(r, 0, RS) {
        const int i = r * G + li;
        if (i < NS) { rec[8 + i] = y[r]; rec[8 + NS + i] = yd[r]; }
    } SEND
}
#endif

#if SA_COMPACT
DEV void store_point(double *rec, int lane, int order, double t, const double (&y)[RS])
{
    if (lane == 0) { rec[0] = (double)order; rec[TREC_T] = t; }
    SFOR(r, 0, RS) { const int i = r * G + lane; if (i < NS) rec[TREC_Y + i] = y[r]; } SEND
}
#endif
/* forward: trajectory record of the newest point (see bdf_kernels.hip::store_table) */
DEV void store_table(double *rec, int lane, int order, double dt, const double (&hT)[QMAX + 1],
                     const double (&hY)[QMAX + 1][RS])
{
    double Y[QMAX + 1][RS];
    SFOR(j, 0, (QMAX) + 1) { SFOR(r, 0, RS) Y[j][r] = hY[j][r]; SEND } SEND
    SFOR(i, 1, (QMAX) + 1) {
        SFOR_DOWN(j, QMAX, 1) {
            if constexpr (j >= i) {
                if (j <= order) {
                    double factor = SA_TABLE_DIV(dt, hT[j] - hT[j - i]);
                    SFOR(r, 0, RS) Y[j][r] = factor * (Y[j][r] - Y[j - 1][r]); SEND
                }
            }
        } SEND
    } SEND
    if (lane == 0) {
        rec[0] = (double)order;
        rec[1] = dt;
        SFOR(j, 0, (QMAX) + 1) rec[2 + j] = hT[j]; SEND
    }
    SFOR(r, 0, RS) {
        const int i = r * G + lane;
        if (i < NS) { SFOR(j, 0, (QMAX) + 1) rec[8 + j * NS + i] = Y[j][r]; SEND }
    } SEND
}

/* ------------------------------------------------------------------------------------ */
/* the kernel body for both launch forms: SA_PT = per-instance start times / output grids (sa_*_batch_times;
   sa_common.h SA_T0 ...), the shared-time kernel otherwise */
template <bool SA_PT>
DEV void k_forward(const sa_fwd_args &a)
{
    const int inst = blockIdx.x * KPW + sa_grp();
    if (inst >= a.B) return;
    if (threadIdx.x == 0) s_nwaves = SA_WAVES;
    if (sa_wave_index() != 0) {
        worker_loop<false>(a.pr + (int64_t)inst * a.rem_stride, ws_inst(a.ws, inst) + WS_OUT);
        return;
    }
    Cw<false> m;
    setup_common(m, a.ps, a.pr, a.rem_stride, inst, a.ws);
    m.rtol = a.rtol;
#ifdef SA_CONSTRAINTS
    m.constr = (a.constraints != nullptr);
    SFOR(r, 0, RS) m.cons[r] = (m.constr && IDX(m, r) < NS) ? a.constraints[IDX(m, r) < NS ? IDX(m, r) : 0] : 0.0; SEND
#endif
    SFOR(r, 0, RS) m.atol[r] = (IDX(m, r) < NS) ? a.atol[IDX(m, r) < NS ? IDX(m, r) : 0] : 1.0; SEND
    m.rtolQ = 0.0; m.atolQ = 1.0; m.tstop = 0.0;
    m.np = 0; m.tfinal = 0.0; m.ilast = 0; m.newdata = 0; m.have_last = 0; m.cur_idx = 0;
    m.last_t = 0.0; m.tlo = m.thi = m.tlo2 = 0.0; m.n_interp = 0; m.n_rebuild = 0;
    m.traj = nullptr; m.trow = 0;

    double y0[RS], q0[RQ];
    SFOR(r, 0, RS) y0[r] = (IDX(m, r) < NS) ? a.y0[(int64_t)inst * NS + (IDX(m, r) < NS ? IDX(m, r) : 0)] : 0.0; SEND
    SFOR(r, 0, RQ) q0[r] = 0.0; SEND
    cv_reinit(m, SA_T0(a, inst), y0, q0);

    /* store: CVodeF semantics (every step is a data point, no mxstep budget); wr: the points are written to the
       arena (SA_MODE_ADJ_COUNT runs the identical pass and only counts them, see sunode_amd.cpp) */
    const bool store = (a.mode != SA_MODE_PLAIN), wr = (a.mode == SA_MODE_ADJ_FWD);
    double *yo = a.y_out + (int64_t)inst * a.n_t * NS;
    double *trec = a.traj + (int64_t)inst * a.traj_istride * TREC;
    const int64_t trow = a.traj_stride * TREC;
    double hT[QMAX + 1], hY[QMAX + 1][RS];
    SFOR(j, 0, (QMAX) + 1) { hT[j] = 0.0; SFOR(r, 0, RS) hY[j][r] = 0.0; SEND } SEND

    int status = CV_SUCCESS, k = 0, np = 0, nstloc = 0, retries = 0, total_retries = 0, attempts = 0;
    while (k < a.n_t && SA_TV(a, inst, k) == SA_T0(a, inst)) {
        SFOR(r, 0, RS) { if (IDX(m, r) < NS) yo[(int64_t)k * NS + IDX(m, r)] = y0[r]; } SEND
        k++;
    }
    bool done = (k >= a.n_t);
    StepCtl c;
    c.in_step = 0; c.redo = 0; c.nflag = FIRST_CALL; c.ncf = c.nef = c.nefQ = 0; c.ncfS = c.nefS = 0; c.convfail = 0; c.saved_t = SA_T0(a, inst);
    if (!done) {
        int flag = cv_first_call(m, SA_TV(a, inst, k));
        if (flag != CV_SUCCESS) { status = flag; done = true; }
        else if (store) {
            hT[0] = m.tn;
            SFOR(r, 0, RS) hY[0][r] = m.zn[0][r]; SEND
#ifdef SA_HERMITE
            if (wr) store_hermite(trec, m.li, m.tn, m.zn[0], m.f0);
#elif SA_COMPACT
            if (wr) store_point(trec, m.li, 0, m.tn, m.zn[0]);
#else
            if (wr) store_table(trec, m.li, 0, 1.0, hT, hY);
#endif
            np = 1;
        }
    }
    while (!done) {
        if (!c.in_step) {
            PH_T0
            int ier = cv_pre_step(m);
            PH_ADD(m, 0)
            if (ier == CV_ILL_INPUT) { status = ier; done = true; }
            else if (!store && a.mxstep > 0 && nstloc >= a.mxstep) {
                retries++; total_retries++;
                if (retries >= a.max_retries) { status = CV_TOO_MUCH_WORK; done = true; }
                else nstloc = 0;
            }
            if (!done && ier != CV_SUCCESS) { status = ier; done = true; }
        }
        if (!done) {
            attempts++;
            int r = cv_attempt(m, c);
            if (r < 0) { status = r; done = true; }
            else if (r == 1) {
                nstloc++;
                if (store) {
                    if (np >= a.traj_max) { status = SA_TRAJ_FULL; done = true; }    /* bounded in every store mode */
                    else {
                        SFOR_DOWN(j, QMAX, 1) { hT[j] = hT[j - 1]; SFOR(s, 0, RS) hY[j][s] = hY[j - 1][s]; SEND } SEND
                        hT[0] = m.tn;
                        SFOR(s, 0, RS) hY[0][s] = m.zn[0][s]; SEND
#ifdef SA_HERMITE
                        {
                            double ydp[RS];
                            SFOR(s, 0, RS) ydp[s] = (1.0 / m.h) * m.zn[1][s]; SEND
                            if (wr && np < a.traj_cap) store_hermite(trec + (int64_t)np * trow, m.li, m.tn, m.zn[0], ydp);
                        }
#elif SA_COMPACT
                        if (wr && np < a.traj_cap) store_point(trec + (int64_t)np * trow, m.li, m.qu, m.tn, m.zn[0]);
#else
                        if (wr && np < a.traj_cap) store_table(trec + (int64_t)np * trow, m.li, m.qu, fabs(hT[0] - hT[1]), hT, hY);
#endif
                        np++;
                    }
                }
                while (!done && k < a.n_t) {
                    double tout = SA_TV(a, inst, k);
                    if (tout == SA_T0(a, inst)) {
                        SFOR(s, 0, RS) { if (IDX(m, s) < NS) yo[(int64_t)k * NS + IDX(m, s)] = y0[s]; } SEND
                        k++;
                    } else if ((m.tn - tout) * m.h >= 0.0) {
                        double dky[RS], dq[RQ];
                        cv_get_dky0(m, tout, dky, dq);
                        SFOR(s, 0, RS) { if (IDX(m, s) < NS) yo[(int64_t)k * NS + IDX(m, s)] = dky[s]; } SEND
                        k++;
                        nstloc = 0; retries = 0;
                    } else break;
                }
                if (k >= a.n_t) done = true;
            }
        }
    }
    release_workers(m);
    if (status != CV_SUCCESS) {
        for (int j = m.li; j < a.n_t * NS; j += G) yo[j] = SA_NAN;
    }
    if (m.li == 0) {
        a.status[inst] = status;
        if (store) {
            a.traj_np[inst] = (status == CV_SUCCESS) ? np : 0;
            /* outgrew the rows of this launch (nothing written beyond them): the host re-integrates exactly sized */
            if (wr && status == CV_SUCCESS && np > a.traj_cap)
                (void)__hip_atomic_fetch_max(a.overflow, np, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        int64_t st[SA_N_STATS];
        SFOR(i, 0, SA_N_STATS) st[i] = 0; SEND
        accumulate_stats(m, st);
        st[ST_NPTS] = np; st[ST_RETRIES] = total_retries; st[ST_ATTEMPTS] = attempts;
#ifdef SA_WAVE_PROFILE
        SFOR(i, 0, 6) st[9 + i] = m.prof[i]; SEND
        st[15] = m.prof[7] + (int64_t)wall_clock64();
#endif
        SFOR(i, 0, SA_N_STATS) a.stats[(int64_t)inst * SA_N_STATS + i] = st[i]; SEND
    }
}
extern "C" __global__ void __launch_bounds__(64 * SA_WAVES) sa_k_forward(sa_fwd_args a) { k_forward<false>(a); }
extern "C" __global__ void __launch_bounds__(64 * SA_WAVES) sa_k_forward_t(sa_fwd_args a) { k_forward<true>(a); }

#ifdef SA_SENS
/* Solver(sens_mode=...).solve (reference solver.py:360-392, 497-531) in the lean lane groups: the forward problem
   together with its NQ sensitivity systems.  Same control flow as sa_k_forward without the trajectory; bit-identical
   to the register kernel's / bdf_mem.hip's sa_k_sens (and to the oracle). */
/* the kernel body for both launch forms: SA_PT = per-instance start times / output grids (sa_*_batch_times;
   sa_common.h SA_T0 ...), the shared-time kernel otherwise */
template <bool SA_PT>
DEV void k_sens(const sa_sens_args &a)
{
    const int inst = blockIdx.x * KPW + sa_grp();
    if (inst >= a.B) return;
    if (threadIdx.x == 0) s_nwaves = 1;
    Cw<false> m;
    setup_common(m, a.ps, a.pr, a.rem_stride, inst, a.ws);
    m.rtol = a.rtol;
#ifdef SA_CONSTRAINTS
    m.constr = 0;
    SFOR(r, 0, RS) m.cons[r] = 0.0; SEND
#endif
    SFOR(r, 0, RS) m.atol[r] = (IDX(m, r) < NS) ? a.atol[IDX(m, r) < NS ? IDX(m, r) : 0] : 1.0; SEND
    m.rtolQ = 0.0; m.atolQ = 1.0; m.tstop = 0.0;
    m.np = 0; m.tfinal = 0.0; m.ilast = 0; m.newdata = 0; m.have_last = 0; m.cur_idx = 0;
    m.last_t = 0.0; m.tlo = m.thi = m.tlo2 = 0.0; m.n_interp = 0; m.n_rebuild = 0;
    m.traj = nullptr; m.trow = 0;
    m.sensi = 1; m.ism = a.ism; m.pbar = a.pbar;

    double y0[RS], q0[RQ];
    SFOR(r, 0, RS) y0[r] = (IDX(m, r) < NS) ? a.y0[(int64_t)inst * NS + (IDX(m, r) < NS ? IDX(m, r) : 0)] : 0.0; SEND
    SFOR(r, 0, RQ) q0[r] = 0.0; SEND
    cv_reinit(m, SA_T0(a, inst), y0, q0);
    const double *s0 = a.sens0 + (int64_t)inst * NQ * NS;
    for (int v = 0; v < SV_COUNT; v++)
        SLOOP_BEGIN(is) SFOR(r, 0, RS) SV(m, v, is, r) = (v == SV_ZN0 && IDX(m, r) < NS) ? s0[is * NS + (IDX(m, r) < NS ? IDX(m, r) : 0)] : 0.0; SEND SLOOP_END

    double *yo = a.y_out + (int64_t)inst * a.n_t * NS;
    double *so = a.sens_out + (int64_t)inst * a.n_t * NQ * NS;
    int status = CV_SUCCESS, k = 0, nstloc = 0, retries = 0, total_retries = 0, attempts = 0;
    while (k < a.n_t && SA_TV(a, inst, k) == SA_T0(a, inst)) {
        SFOR(r, 0, RS) { if (IDX(m, r) < NS) yo[(int64_t)k * NS + IDX(m, r)] = y0[r]; } SEND
        SLOOP_BEGIN(is) SFOR(r, 0, RS) { if (IDX(m, r) < NS) so[((int64_t)k * NQ + is) * NS + IDX(m, r)] = s0[is * NS + IDX(m, r)]; } SEND SLOOP_END
        k++;
    }
    bool done = (k >= a.n_t);
    StepCtl c;
    c.in_step = 0; c.redo = 0; c.nflag = FIRST_CALL; c.ncf = c.nef = c.nefQ = 0; c.ncfS = c.nefS = 0; c.convfail = 0;
    c.saved_t = SA_T0(a, inst);
    if (!done) {
        int flag = cv_first_call(m, SA_TV(a, inst, k));
        if (flag != CV_SUCCESS) { status = flag; done = true; }
    }
    while (!done) {
        if (!c.in_step) {
            int ier = cv_pre_step(m);
            if (ier == CV_ILL_INPUT) { status = ier; done = true; }
            else if (a.mxstep > 0 && nstloc >= a.mxstep) {
                retries++; total_retries++;
                if (retries >= a.max_retries) { status = CV_TOO_MUCH_WORK; done = true; }
                else nstloc = 0;
            }
            if (!done && ier != CV_SUCCESS) { status = ier; done = true; }
        }
        if (!done) {
            attempts++;
            int r = cv_attempt(m, c);
            if (r < 0) { status = r; done = true; }
            else if (r == 1) {
                nstloc++;
                while (!done && k < a.n_t) {
                    double tout = SA_TV(a, inst, k);
                    if (tout == SA_T0(a, inst)) {
                        SFOR(s, 0, RS) { if (IDX(m, s) < NS) yo[(int64_t)k * NS + IDX(m, s)] = y0[s]; } SEND
                        SLOOP_BEGIN(is) SFOR(s, 0, RS) { if (IDX(m, s) < NS) so[((int64_t)k * NQ + is) * NS + IDX(m, s)] = s0[is * NS + IDX(m, s)]; } SEND SLOOP_END
                        k++;
                    } else if ((m.tn - tout) * m.h >= 0.0) {
                        double dky[RS], dq[RQ];
                        cv_get_dky0(m, tout, dky, dq);
                        SFOR(s, 0, RS) { if (IDX(m, s) < NS) yo[(int64_t)k * NS + IDX(m, s)] = dky[s]; } SEND
                        {   /* CVodeGetSensDky, k = 0 (t validated by cv_get_dky0) */
                            const double sx = (tout - m.tn) / m.h;
                            double pw[QMAX + 1];
                            pw[0] = 1.0;
                            SFOR(j, 1, (QMAX) + 1) pw[j] = pw[j - 1] * sx; SEND
                            SLOOP_BEGIN(is)
                                SFOR(s, 0, RS) {
                                    double acc = pw[QMAX] * SV(m, SV_ZN0 + QMAX, is, s);
                                    SFOR_DOWN(j, QMAX - 1, 0) acc = FMA(pw[j], SV(m, SV_ZN0 + j, is, s), acc); SEND
                                    if (IDX(m, s) < NS) so[((int64_t)k * NQ + is) * NS + IDX(m, s)] = acc;
                                } SEND
                            SLOOP_END
                        }
                        k++;
                        nstloc = 0; retries = 0;
                    } else break;
                }
                if (k >= a.n_t) done = true;
            }
        }
    }
    if (status != CV_SUCCESS) {
        for (int j = m.li; j < a.n_t * NS; j += G) yo[j] = SA_NAN;
        for (int j = m.li; j < a.n_t * NQ * NS; j += G) so[j] = SA_NAN;
    }
    if (m.li == 0) {
        a.status[inst] = status;
        int64_t st[SA_N_STATS];
        SFOR(i, 0, SA_N_STATS) st[i] = 0; SEND
        accumulate_stats(m, st);
        /* sensitivity counters ride in the quadrature / interpolation slots of the adjoint path */
        st[ST_NFQE] = m.nfSe; st[ST_NETFQ] = m.netfS; st[ST_NINTERP] = m.nniS; st[ST_NREBUILD] = m.ncfnS;
        st[ST_RETRIES] = total_retries; st[ST_ATTEMPTS] = attempts;
        SFOR(i, 0, SA_N_STATS) a.stats[(int64_t)inst * SA_N_STATS + i] = st[i]; SEND
    }
}
extern "C" __global__ void __launch_bounds__(64) sa_k_sens(sa_sens_args a) { k_sens<false>(a); }
extern "C" __global__ void __launch_bounds__(64) sa_k_sens_t(sa_sens_args a) { k_sens<true>(a); }
#endif

/* the kernel body for both launch forms: SA_PT = per-instance start times / output grids (sa_*_batch_times;
   sa_common.h SA_T0 ...), the shared-time kernel otherwise */
template <bool SA_PT>
DEV void k_backward(const sa_bwd_args &a)
{
    const int inst = blockIdx.x * KPW + sa_grp();
    if (inst >= a.B) return;
    if (threadIdx.x == 0) s_nwaves = SA_WAVES;
#if defined(SA_WAVE_PROFILE) && SA_WAVES > 1
    if (threadIdx.x == 0) { for (int i = 0; i < 12; i++) s_luprof[i] = 0; }
#endif
    if (sa_wave_index() != 0) {
        worker_loop<true>(a.pr + (int64_t)inst * a.rem_stride, ws_inst(a.ws, inst) + WS_OUT);
        return;
    }
    /* Little stays live across the step loops of an interval: the counters of finished intervals accumulate in the
       instance's row of the stats array, the adjoint state / quadrature between two intervals wait in the output rows
       (lamda_out / grad_out are ours until the kernel ends) -- ~50 registers the Newton pass does not have to spill. */
    int64_t *strow = a.stats + (int64_t)inst * SA_N_STATS;
    int status = CV_SUCCESS;
    const int np = a.traj_np[inst];
    if (a.fwd_status[inst] != CV_SUCCESS || np < 2) status = CV_NO_FWD;

    Cw<true> m;
    setup_common(m, a.ps, a.pr, a.rem_stride, inst, a.ws);
    m.rtol = a.rtolB;
    SFOR(r, 0, RS) m.atol[r] = a.atolB; SEND
    m.rtolQ = a.rtolQB; m.atolQ = a.atolQB;
    m.tstop = SA_TINIT(a, inst);
    m.traj = a.traj + (int64_t)inst * a.traj_istride * TREC;
    m.trow = a.traj_stride * TREC;
    m.np = np;
    m.tfinal = (status == CV_SUCCESS) ? m.traj[(int64_t)(np - 1) * m.trow + TREC_T] : SA_TINIT(a, inst);
    m.cur_idx = 0; m.tlo2 = 0.0; m.tlo = m.thi = 0.0;
    m.ilast = 0; m.newdata = 1; m.have_last = 0; m.last_t = 0.0;
    m.n_interp = 0; m.n_rebuild = 0;

    double *lam_g = a.lamda_out + (int64_t)inst * NS, *quad_g = a.grad_out + (int64_t)inst * NQ;
    {
        double lam0[RS], quad0[RQ];
        SFOR(r, 0, RS) { lam0[r] = 0.0; if (IDX(m, r) < NS) lam_g[IDX(m, r)] = 0.0; } SEND
        SFOR(r, 0, RQ) { quad0[r] = 0.0; if (IDX(m, r) < NQ) quad_g[IDX(m, r)] = 0.0; } SEND
        if (m.li == 0) { SFOR(i, 0, SA_N_STATS) strow[i] = 0; SEND }
        cv_reinit(m, SA_T0(a, inst), lam0, quad0);
    }
    const double *g = a.grads + (int64_t)inst * a.grads_stride;
    bool first_call = true;
    int total_retries = 0, attempts = 0;

    for (int iv = 0; iv <= a.n_t; iv++) {
        const double t_upper = (iv == 0) ? SA_T0(a, inst) : SA_TV(a, inst, a.n_t - iv);
        const double t_lower = (iv == a.n_t) ? SA_TEND(a, inst) : SA_TV(a, inst, a.n_t - 1 - iv);
        if (t_lower < t_upper) {
            if (status == CV_SUCCESS) {
                {
                    double lam[RS], quad[RQ];
                    SFOR(r, 0, RS) lam[r] = (IDX(m, r) < NS) ? lam_g[IDX(m, r) < NS ? IDX(m, r) : 0] : 0.0; SEND
                    SFOR(r, 0, RQ) quad[r] = (IDX(m, r) < NQ) ? quad_g[IDX(m, r) < NQ ? IDX(m, r) : 0] : 0.0; SEND
                    cv_reinit(m, t_upper, lam, quad);
                }
                if (first_call) {
                    if ((t_upper - SA_TINIT(a, inst)) < 0.0 || (m.tfinal - t_upper) < 0.0) status = CV_BAD_TB0;
                    first_call = false;
                }
                if (status == CV_SUCCESS && ((t_lower - SA_TINIT(a, inst)) < 0.0 || (m.tfinal - t_lower) < 0.0)) {
                    double tfuzz = 100.0 * UROUND * (fabs(SA_TINIT(a, inst)) + fabs(m.tfinal));
                    if ((t_lower - SA_TINIT(a, inst)) < -tfuzz || (m.tfinal - t_lower) < -tfuzz) status = CV_ILL_INPUT;
                }
                if (status == CV_SUCCESS) {
                    PH_T0
                    int flag = cv_first_call(m, t_lower);
                    PH_ADD(m, 6)
                    if (flag != CV_SUCCESS) status = flag;
                }
            }
            int nstloc = 0, retries = 0;
            StepCtl c;
            c.in_step = 0; c.redo = 0; c.nflag = FIRST_CALL; c.ncf = c.nef = c.nefQ = 0; c.ncfS = c.nefS = 0; c.convfail = 0;
            c.saved_t = t_upper;
            bool idone = (status != CV_SUCCESS);
            while (!idone) {
                if (!c.in_step) {
                    PH_T0
                    int ier = cv_pre_step(m);
                    PH_ADD(m, 0)
                    if (ier == CV_ILL_INPUT) { status = ier; idone = true; }
                    else if (a.mxstep > 0 && nstloc >= a.mxstep) {
                        retries++; total_retries++;
                        if (retries >= a.max_retries) { status = CV_TOO_MUCH_WORK; idone = true; }
                        else nstloc = 0;
                    }
                    if (!idone && ier != CV_SUCCESS) { status = ier; idone = true; }
                }
                if (!idone) {
                    attempts++;
                    int r = cv_attempt(m, c);
                    if (r < 0) { status = r; idone = true; }
                    else if (r == 1) {
                        nstloc++;
                        double troundoff = FUZZ_FACTOR * UROUND * (fabs(m.tn) + fabs(m.h));
                        if (fabs(m.tn - m.tstop) <= troundoff) m.tn = m.tstop;
                        if ((m.tn - t_lower) * m.h >= 0.0) {
                            double lam[RS], quad_out[RQ];
                            cv_get_dky0(m, t_lower, lam, quad_out);
                            SFOR(r, 0, RS) { if (IDX(m, r) < NS) lam_g[IDX(m, r)] = lam[r]; } SEND
                            SFOR(r, 0, RQ) { if (IDX(m, r) < NQ) quad_g[IDX(m, r)] = quad_out[r]; } SEND
                            idone = true;
                        } else {
                            troundoff = FUZZ_FACTOR * UROUND * (fabs(m.tn) + fabs(m.h));
                            if (fabs(m.tn - m.tstop) <= troundoff) { status = CV_TSTOP_RETURN; idone = true; }
                            else if ((m.tn + m.hprime - m.tstop) * m.h > 0.0) {
                                m.hprime = (m.tstop - m.tn) * (1.0 - 4.0 * UROUND);
                                m.eta = m.hprime / m.h;
                            }
                        }
                    }
                }
            }
            if ((status == CV_SUCCESS || m.nst > 0) && m.li == 0) {
                int64_t st[SA_N_STATS];
                SFOR(i, 0, SA_N_STATS) st[i] = strow[i]; SEND
                accumulate_stats(m, st);
                SFOR(i, 0, SA_N_STATS) strow[i] = st[i]; SEND
            }
        }
        if (iv < a.n_t && status == CV_SUCCESS) {
            const double *gi = g + (int64_t)(a.n_t - 1 - iv) * NS;
            const int64_t row = (int64_t)inst * a.n_t + (iv == 0 ? 0 : a.n_t - iv);
            SFOR(r, 0, RS) {
                if (IDX(m, r) < NS) {
                    const double v = lam_g[IDX(m, r)] - gi[IDX(m, r)];
                    lam_g[IDX(m, r)] = v;
                    if (a.lamda_all) a.lamda_all[row * NS + IDX(m, r)] = v;
                }
            } SEND
            if (a.quad_all) { SFOR(r, 0, RQ) { if (IDX(m, r) < NQ) a.quad_all[row * NQ + IDX(m, r)] = quad_g[IDX(m, r)]; } SEND }
        }
    }
    release_workers(m);
    if (status != CV_SUCCESS) {
        if (a.lamda_all) for (int j = m.li; j < a.n_t * NS; j += G) a.lamda_all[(int64_t)inst * a.n_t * NS + j] = SA_NAN;
        if (a.quad_all) for (int j = m.li; j < a.n_t * NQ; j += G) a.quad_all[(int64_t)inst * a.n_t * NQ + j] = SA_NAN;
    }
    if (status != CV_SUCCESS) {
        SFOR(r, 0, RQ) { if (IDX(m, r) < NQ) quad_g[IDX(m, r)] = SA_NAN; } SEND
        SFOR(r, 0, RS) { if (IDX(m, r) < NS) lam_g[IDX(m, r)] = SA_NAN; } SEND
    }
    if (m.li == 0) {
        a.status[inst] = status;
        int64_t st[SA_N_STATS];
        SFOR(i, 0, SA_N_STATS) st[i] = strow[i]; SEND
        st[ST_NPTS] = np; st[ST_NINTERP] = m.n_interp; st[ST_NREBUILD] = m.n_rebuild;
        st[ST_RETRIES] = total_retries; st[ST_ATTEMPTS] = attempts;
#ifdef SA_WAVE_PROFILE
        SFOR(i, 0, 6) st[9 + i] = m.prof[i]; SEND
        st[15] = m.prof[7] + (int64_t)wall_clock64();
#if defined(SA_WAVE_PROFILE_PHASES) && SA_WAVES == 1
        st[ST_NPTS] = m.prof[6];            /* phase builds: restarts (cv_first_call: f, fQ, cvHin) in the point-count slot */
#endif
#if SA_WAVES > 1
        st[5] = s_luprof[0]; st[6] = s_luprof[1]; st[7] = s_luprof[2];      /* LU: cycles pre-barrier / barrier / update */
        st[8] = s_luprof[3] + (s_luprof[4] << 32);                          /* ... prologue | epilogue << 32 */
#ifdef SA_LU_PROFILE_SEGMENTS       /* load + form | first barrier | write-back | last barrier, cycles (replace the section slots) */
        st[9] = s_luprof[5]; st[10] = s_luprof[6]; st[11] = s_luprof[7]; st[12] = s_luprof[8];
        st[13] = s_luprof[9]; st[14] = s_luprof[10];        /* owner block: update of its four columns | the four steps */
#endif
#ifdef SA_LU_PROFILE_TIMELINE
        st[13] = s_luprof[11]; st[14] = blockIdx.x % LU_NPANEL;
#endif
#endif
#endif
        SFOR(i, 0, SA_N_STATS) a.stats[(int64_t)inst * SA_N_STATS + i] = st[i]; SEND
    }
}
extern "C" __global__ void __launch_bounds__(64 * SA_WAVES) sa_k_backward(sa_bwd_args a) { k_backward<false>(a); }
extern "C" __global__ void __launch_bounds__(64 * SA_WAVES) sa_k_backward_t(sa_bwd_args a) { k_backward<true>(a); }

/* callback evaluation: the host launches ceil(npts/64) blocks; a block walks its 64 points with
   the whole wave (inputs staged in LDS exactly as in the integrator) */
struct ArrayOut {
    gdouble *p;
    template <int S> __device__ __forceinline__ void put(double x) const { p[S] = x; }
    __device__ __forceinline__ void put_dyn(int slot, double x) const { p[slot] = x; }
};

extern "C" __global__ void __launch_bounds__(64) sa_k_eval(sa_eval_args a)
{
    const int lane = lane_id(), li = lane & (G - 1), grp = lane / G;
    if (lane == 0) s_nwaves = 1;
    for (int q = 0; q < G; q++) {                 /* every group of the wavefront walks its own points */
        const int i = blockIdx.x * 64 + q * KPW + grp;
        if (i >= a.npts) break;
        lds_sync();
        for (int k = li; k < NS; k += G) {
            s_y[grp * W_NSP + k] = a.y[(int64_t)i * NS + k];
            s_lam[grp * W_NSP + k] = a.lam[(int64_t)i * NS + k];
        }
        for (int k = li; k < NQ; k += G) s_ps[grp * W_NQP + k] = a.ps[(int64_t)i * NQ + k];
        lds_sync();
        const double *prp = a.pr + (int64_t)i * NR;
        const double t = a.t[i];
        const int c0 = sa_rhs(t, nullptr, nullptr, prp, ArrayOut{(gdouble *)(a.rhs + (int64_t)i * NS)});
        const int c1 = sa_jac(t, nullptr, nullptr, prp, ArrayOut{(gdouble *)(a.jac + (int64_t)i * NS * NS)});
        const int c2 = sa_adj_rhs(t, nullptr, nullptr, nullptr, prp, ArrayOut{(gdouble *)(a.adj + (int64_t)i * NS)});
        const int c3 = sa_quad_rhs(t, nullptr, nullptr, nullptr, prp, ArrayOut{(gdouble *)(a.quad + (int64_t)i * NQ)});
        const int c4 = sa_adj_jac(t, nullptr, nullptr, prp, ArrayOut{(gdouble *)(a.adjjac + (int64_t)i * NS * NS)});
        if (li == 0) {
            a.codes[i * 5 + 0] = c0; a.codes[i * 5 + 1] = c1; a.codes[i * 5 + 2] = c2;
            a.codes[i * 5 + 3] = c3; a.codes[i * 5 + 4] = c4;
        }
    }
}

extern "C" __global__ void __launch_bounds__(64) sa_k_math(sa_math_args a)
{
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= a.n) return;
    {   /* both coefficient sources of the deterministic pow (literals / constant memory, sa_common.h) must agree bit for bit */
        const double plit = rpower_r<false>(a.x[i], a.y[i]), pcm = rpower_r<true>(a.x[i], a.y[i]);
        a.pow_out[i] = (__builtin_bit_cast(uint64_t, plit) == __builtin_bit_cast(uint64_t, pcm)) ? plit : SA_NAN;
    }
    a.sqrt_out[i] = sqrt(a.x[i]);
    {   /* odd entries with operands far from the exponent limits go through fdiv (cvSet's division): the host test
           compares every entry with the IEEE quotient */
        const double xa = fabs(a.x[i]), ya = fabs(a.y[i]);
        const bool safe = (i & 1) && xa > 1e-100 && xa < 1e100 && ya > 1e-100 && ya < 1e100;
        a.div_out[i] = safe ? fdiv(a.x[i], a.y[i]) : a.x[i] / a.y[i];
    }
}

/* {n_states, n_sub, n_rem, ABI version, lanes per instance, workspace doubles per instance} */
#if SA_COMPACT
extern "C" __device__ __attribute__((used)) const int32_t sa_traj_rec = TREC;
#endif
extern "C" __device__ __attribute__((used)) const int32_t sa_meta[6] = {NS, NQ, NR, SA_DEVICE_ABI_VERSION, G * SA_WAVES, WS_DOUBLES};
