// Streaming form of the fused E -> B/G -> D -> B^T/G^T -> E^T kernel for Nedelec hexahedra with THREE points per
// direction (p = 2 on its own rule -- 27 points, 54 dofs per element -- and its p-coarsened level) on packed q-data.
// Opt-in: PALACE_AMD_STREAM3=1 at operator creation (nd_hex_stream3_ok); the default at three points stays the one-shot
// kernel nd_hex_apply_kernel (pa_nd_hex.hip).
//
// Same arithmetic as nd_hex_apply_kernel (the passes of pa_nd_hex_core.hpp on NDTab<P1, 3>; reference
// fem/libceed/operator.cpp:148-178 and the QFunctions fem/qfunctions/33/{hdiv_33,hcurl_33,hdivmass_33}_qf.h) and the same
// schedule as nd_hex_stream_kernel (pa_nd_hex_stream.hip): persistent waves walk the batches of one XCD's contiguous element
// range with a fixed stride and keep the HBM streams of the NEXT batch in flight while they compute the current one:
//   top of batch i                          q-data of batch i, index and flag words of batch i + 1
//   E stage, forward passes, D              ...
//   after the first transposed component    slot words and x[index] of batch i + 1 (its index words have arrived by now)
//   the other transposed components, E^T stores
// The element-local results are signed and stored once, exclusive dofs straight to y, the others to the E-vector that
// et_run_gather_kernel sums by runs in fixed order.
//
// Mapping: sixteen lanes per element and four elements per wave, as at four points per direction, so that every host table
// of that kernel is used as it is (streamhost::pack_index, the [ne][16] flag words, the dictionary of slot patterns, the run
// lists, their masked and `all` copies, SplitIO).  Lanes t < 9 of an element own the columns (t % 3, t / 3) of its 27 points
// in the contraction passes and the D stage; all sixteen take part in E / E^T with entries m = t + 16 r of the sorted dof list
// (p = 2: four entries per lane, 54 in all; p = 1: one entry on twelve lanes).  The seven lanes without a column run the
// passes on lane 0's addresses with their stores switched off (lane_ok): flops the kernel, bound by its streams, does not miss.
// What differs from the four-point kernel besides the rule:
//   * q-data [ncomp][27] per element (nd_qd_offset: the general layout, the one the one-shot kernel reads): a lane reads the
//     three points of its column with three 8-byte loads per component, nine lanes cover 72 contiguous bytes;
//   * no compact-D batches (affine / column), no geometry from the nodes, no one-pass complex form, no request of the q-data
//     one batch ahead: the flag words of a three-point block never carry kAffBit / kColBit (stream_affine_setup leaves other
//     rules alone).
#include <algorithm>

#include "pa_nd_hex_core.hpp"
#include "pa_stream_launch.hpp"

namespace pa {

typedef double d2v3 __attribute__((ext_vector_type(2)));

// Element stride in LDS (doubles): the bank rule at the top of pa_nd_hex_stream.hip (stream_lds_elem) -- the two elements of a
// 32-lane read group have to sit 16 (mod 32) doubles apart.  The dense contraction layouts NDLayout<P1, 3> touch, per element
// and instruction, either nine consecutive doubles (pass X stores, pass Z loads and their transposes) or three groups of three,
// nine doubles apart (pass Y and its transpose at p = 2: offsets {0, 1, 2, 9, 10, 11, 18, 19, 20}).  At 16 (mod 32) the first
// kind is conflict-free; the second shares two of its nine banks with the other element's image (18 and 2), i.e. those
// instructions take two cycles instead of one.  No stride serves both kinds: the first needs a shift in [9, 23], the second one
// in {3..6, 26..29}.
__host__ __device__ constexpr int stream3_lds_elem(const int raw) { return (raw + 15) / 32 * 32 + 16; }

template <int P1>
struct NDStream3Args {
  int ne, nbatch, chunk;  // chunk: batches per XCD (contiguous range)
  const uint32_t *idxc;   // [nep][kIdxWords] run-compressed sorted element -> dof index (pa_stream_host.hpp)
  const uint32_t *flagw;  // [nep][16]: bit 2 r = entry t + 16 r is flipped, bit 2 r + 1 = it is the only copy of its dof,
                          // bit 18 + r = essential (read as zero; set in the copies used by the masked applies)
  const uint32_t *slots;  // [patterns][NPK][16]: four 8-bit tensor-order slots per word; an element names its pattern in word
                          // kIdxPattern of its index block (pa_nd_hex_stream.hip: build_stream)
  const double *qdata;    // [nep][NG][27]
  const double *coef;     // metric form: [nep][2] scalar mass / curl-curl coefficient of the element
  const double *x;
  double *y, *ye;
  // split vectors (SPLIT; NDStreamArgs in pa_nd_hex_stream.hip): ghosts [nsplit, lsize) read from xg0 | xg1 (parity of *xg_sel),
  // written to yg; the three pointers are stored shifted by -nsplit
  int nsplit;
  const double *xg0, *xg1;
  const unsigned long long *xg_sel;
  double *yg;
  NDTab<P1, 3> tab;
};

// METRIC: q-data = (w / |detJ|) J^T J and |detJ| / w (7 doubles per point, 6 read by the curl-curl kernel), the scalar
// coefficients of the element applied here; else packed symmetric D, six rows per term (mass rows first).
// MINW: waves per SIMD the instantiation is compiled for.
template <int P1, bool USE_U, bool USE_C, bool METRIC, int MINW, bool SPLIT = false>
__global__ __launch_bounds__(64 * kWavesPerBlock, MINW) void nd_hex_stream3_kernel(const NDStream3Args<P1> a) {
  constexpr int Q1 = 3;
  using L = NDLayout<P1, Q1>;
  constexpr int NC = P1 + 1, PP = 3 * P1 * NC * NC, NPL = (PP + 15) / 16, NPK = (NPL + 3) / 4;
  constexpr int NG = METRIC ? (USE_U ? 7 : 6) : 6 * ((USE_U ? 1 : 0) + (USE_C ? 1 : 0));
  constexpr int CS = Q1 * Q1 * Q1;  // nd_qd_cstride(3)
  static_assert(P1 <= 2 && PP <= L::ELEM, "the tensor-order dofs are staged in the contraction buffers");
  using streamhost::kIdxPattern;
  using streamhost::kIdxStart0;
  using streamhost::kIdxWords;
  // LDS per element (doubles): contraction buffers + the batch's index and slot / flag words, kept for the E^T stores,
  // + the run starts of the next batch while its index is decoded (20 ints)
  constexpr int LDS_SIDE = (PP + 1) / 2 + (NPK + 1) * 8;
  constexpr int LDS_ELEM = stream3_lds_elem(L::ELEM_PAD + LDS_SIDE + 12);
  extern __shared__ __attribute__((aligned(16))) double smem[];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  // XCD k (workgroups are dealt to the XCDs round-robin) owns the batches [k chunk, (k + 1) chunk); its waves walk them with
  // a fixed stride
  const int xcd = blockIdx.x & 7;
  const int base = xcd * a.chunk, bend = min(base + a.chunk, a.nbatch);
  const int stride = (int)(gridDim.x >> 3) * kWavesPerBlock;
  int b = base + (int)(blockIdx.x >> 3) * kWavesPerBlock + wave;
  if (b >= bend) return;
  const double *xgh = nullptr;  // SPLIT: where the ghost entries are read (shifted: indexed with the local dof)
  if (SPLIT) xgh = ((a.xg_sel ? *a.xg_sel : 0ull) & 1ull) ? a.xg1 : a.xg0;
  // index words of a batch (every array is padded to a multiple of four elements; pad entries read as zero and are stored to
  // E-vector rows nobody gathers): s[0 .. NPL) the slice words, s[NPL], s[NPL + 1] run starts t, 16 + (t & 3); p[NPK] the flag
  // word, p[0] the pattern number until the slot words replace it (gather)
  auto load_idx = [&](const int bb, const int sub, const int t, int (&s)[NPL + 2], unsigned (&p)[NPK + 1]) {
    const int e = bb * 4 + sub;
    const uint32_t *ic = a.idxc + (size_t)e * kIdxWords;
#pragma unroll
    for (int r = 0; r < NPL; r++) s[r] = (int)__builtin_nontemporal_load(&ic[r]);
    s[NPL] = (int)__builtin_nontemporal_load(&ic[kIdxStart0 + t]);
    s[NPL + 1] = (int)__builtin_nontemporal_load(&ic[kIdxStart0 + 16 + (t & 3)]);
    p[NPK] = __builtin_nontemporal_load(&a.flagw[(size_t)e * 16 + t]);
    p[0] = __builtin_nontemporal_load(&ic[kIdxPattern]);
  };
  // decodes the index of the batch in place (s[r] becomes dof | kEssBit | kExclBit, negative: -(1 + word), flipped) and
  // requests the raw x of the entries (essential entries are zeroed when staged).  stab: 20 ints of LDS of this element.
  auto gather = [&](int (&s)[NPL + 2], unsigned (&p)[NPK + 1], double (&xv)[NPL], int *stab, const int t) {
    stab[t] = s[NPL];
    if (t < 4) stab[16 + t] = s[NPL + 1];
    wave_sync();
    const unsigned fw = p[NPK];
    {
      const uint32_t *sl = a.slots + (size_t)p[0] * (NPK * 16) + t;
#pragma unroll
      for (int k = 0; k < NPK; k++) p[k] = sl[16 * k];
    }
#pragma unroll
    for (int r = 0; r < NPL; r++) {
      const unsigned w = (unsigned)s[r], low = (w & 0xffffu) & ((2u << t) - 1u);
      const int rid = (int)((w >> 16) & 31u) + __popc(low) - 1;
      const int pos = low ? 16 * r + 31 - __clz((int)low) : (int)((w >> 21) & 255u);
      int dof = stab[rid] + (t + 16 * r - pos);
      if (!(16 * r + 15 < PP) && t + 16 * r >= PP) dof = 0;  // lanes past the last entry
      xv[r] = SPLIT ? (dof < a.nsplit ? a.x : xgh)[dof] : a.x[dof];
      const int word = dof | ((fw >> (2 * r + 1)) & 1u ? kExclBit : 0) | ((fw >> (18 + r)) & 1u ? kEssBit : 0);
      s[r] = (fw >> (2 * r)) & 1u ? -1 - word : word;
    }
  };
  // (the flag word is taken as arrived before the loop / behind the gather: see nd_hex_stream_kernel)
  auto settle = [&](unsigned (&p)[NPK + 1]) { asm volatile("" : "+v"(p[NPK])); };
  int sA[NPL + 2];
  unsigned pA[NPK + 1];
  double xv[NPL];
  load_idx(b, lane >> 4, lane & 15, sA, pA);
  gather(sA, pA, xv, reinterpret_cast<int *>(smem + (size_t)(wave * 4 + (lane >> 4)) * LDS_ELEM + L::ELEM_PAD + LDS_SIDE), lane & 15);
  // the first batch's x is awaited outside the loop (nd_hex_stream_kernel: the counted waits at the top of every batch)
#pragma unroll
  for (int r = 0; r < NPL; r++) asm volatile("" : "+v"(xv[r]));
  settle(pA);

  for (;;) {
    // lane constants re-derived from an opaque copy of the lane id in every iteration (hoisted, the LDS addresses and
    // predicates of the passes stay live across the loop)
    int lo = lane;
    asm volatile("" : "+v"(lo));
    const int sub = lo >> 4, t = lo & 15;
    const bool lane_ok = t < Q1 * Q1;  // owns a column
    const int tc = lane_ok ? t : 0, ta = tc % Q1, tb = tc / Q1;
    double *sm = smem + (size_t)(wave * 4 + sub) * LDS_ELEM;
    int *side = reinterpret_cast<int *>(sm + L::ELEM_PAD);  // index words of this batch, kept for the E^T stores
    int *stab = side + 2 * LDS_SIDE;                        // run starts of the next batch (decode)
    const int e = b * 4 + sub;

    // q-data of this batch: consumed after the forward contraction (read once: non-temporal)
    double gq[NG][Q1];
    {
      const double *g = a.qdata + (size_t)e * ((METRIC ? 7 : NG) * CS) + tc;  // (the metric form always stores 7 per point)
#pragma unroll
      for (int c = 0; c < NG; c++)
#pragma unroll
        for (int qz = 0; qz < Q1; qz++) gq[c][qz] = __builtin_nontemporal_load(&g[c * CS + Q1 * Q1 * qz]);
    }
    d2v3 ce = {0.0, 0.0};
    if (METRIC) ce = reinterpret_cast<const d2v3 *>(a.coef)[e];

    // E: sorted entries into their tensor-order slots (x of this batch was requested during the previous one)
#pragma unroll
    for (int r = 0; r < NPL; r++) {
      if (16 * r + 15 < PP || t + 16 * r < PP) {
        const int sv = sA[r], df = sv >= 0 ? sv : -1 - sv;
        const double v = (df & kEssBit) ? 0.0 : xv[r];
        sm[(pA[r >> 2] >> (8 * (r & 3))) & 255u] = sv >= 0 ? v : -v;
        side[t + 16 * r] = sv;
      }
    }
#pragma unroll
    for (int k = 0; k <= NPK; k++) side[2 * ((PP + 1) / 2) + 16 * k + t] = (int)pA[k];
    wave_sync();
    double uin[3][NC];
#pragma unroll
    for (int C = 0; C < 3; C++) {
      const int ni = (C == 0) ? P1 : NC, nj = (C == 1) ? P1 : NC, nk = (C == 2) ? P1 : NC;
      const bool act = ta < nj && tb < nk;
#pragma unroll
      for (int i = 0; i < NC; i++) uin[C][i] = (act && i < ni) ? sm[C * P1 * NC * NC + i + ni * (ta + nj * tb)] : 0.0;
    }
    wave_sync();

    // index words of the next batch (clamped: the last iteration re-reads its own); first use: the x gather below
    const int kn = b + stride;
    const bool more = kn < bend;
    const int bn = more ? kn : b;
    int sB[NPL + 2];
    unsigned pB[NPK + 1];
    load_idx(bn, sub, t, sB, pB);
    __builtin_amdgcn_sched_barrier(0);

    double U[3][Q1], CU[3][Q1];
#pragma unroll
    for (int c = 0; c < 3; c++)
#pragma unroll
      for (int q = 0; q < Q1; q++) U[c][q] = 0.0, CU[c][q] = 0.0;
    nd_fwd_comp<0, P1, Q1, USE_U, USE_C, L>(a, e, true, lane_ok, ta, tb, 0, sm, uin[0], U, CU);
    nd_fwd_comp<1, P1, Q1, USE_U, USE_C, L>(a, e, true, lane_ok, ta, tb, 0, sm, uin[1], U, CU);
    nd_fwd_comp<2, P1, Q1, USE_U, USE_C, L>(a, e, true, lane_ok, ta, tb, 0, sm, uin[2], U, CU);

    // D at the three points of this lane's column
#pragma unroll
    for (int qz = 0; qz < Q1; qz++) {
      double H[NG];
#pragma unroll
      for (int c = 0; c < NG; c++) H[c] = gq[c][qz];
      if (METRIC) {
        // H = (w / |detJ|) J^T J {00, 01, 02, 11, 12, 22}, H[6] = |detJ| / w:
        //   (w / detJ) J^T c J = c H,   w detJ adj^T c adj = c (|detJ| / w) adj(H)
        if (USE_U) {
          const double cm = H[6] * ce[0];
          const double m[6] = {cm * (H[3] * H[5] - H[4] * H[4]), cm * (H[2] * H[4] - H[1] * H[5]), cm * (H[1] * H[4] - H[2] * H[3]),
                               cm * (H[0] * H[5] - H[2] * H[2]), cm * (H[1] * H[2] - H[0] * H[4]), cm * (H[0] * H[3] - H[1] * H[1])};
          sym_mv(m, U[0][qz], U[1][qz], U[2][qz], U[0][qz], U[1][qz], U[2][qz]);
        }
        if (USE_C) {
          const double m[6] = {ce[1] * H[0], ce[1] * H[1], ce[1] * H[2], ce[1] * H[3], ce[1] * H[4], ce[1] * H[5]};
          sym_mv(m, CU[0][qz], CU[1][qz], CU[2][qz], CU[0][qz], CU[1][qz], CU[2][qz]);
        }
        __builtin_amdgcn_sched_barrier(0);  // one point at a time: short live ranges
      } else {
        if (USE_U) sym_mv(&H[0], U[0][qz], U[1][qz], U[2][qz], U[0][qz], U[1][qz], U[2][qz]);
        if (USE_C) sym_mv(&H[USE_U ? 6 : 0], CU[0][qz], CU[1][qz], CU[2][qz], CU[0][qz], CU[1][qz], CU[2][qz]);
      }
    }

    // x of the next batch: in flight during the rest of the transposed passes
    double xB[NPL];
    nd_bwd_comp<0, P1, Q1, USE_U, USE_C, L>(a, e, true, lane_ok, ta, tb, 0, sm, uin[0], U, CU);
    __builtin_amdgcn_sched_barrier(0);
    gather(sB, pB, xB, stab, t);
    settle(pB);
    __builtin_amdgcn_sched_barrier(0);
    nd_bwd_comp<1, P1, Q1, USE_U, USE_C, L>(a, e, true, lane_ok, ta, tb, 0, sm, uin[1], U, CU);
    nd_bwd_comp<2, P1, Q1, USE_U, USE_C, L>(a, e, true, lane_ok, ta, tb, 0, sm, uin[2], U, CU);

    // E^T: back to tensor order in LDS, out in sorted order, signed; exclusive dofs straight to y
#pragma unroll
    for (int C = 0; C < 3; C++) {
      const int ni = (C == 0) ? P1 : NC, nj = (C == 1) ? P1 : NC, nk = (C == 2) ? P1 : NC;
      const bool act = lane_ok && ta < nj && tb < nk;
#pragma unroll
      for (int i = 0; i < NC; i++)
        if (act && i < ni) sm[C * P1 * NC * NC + i + ni * (ta + nj * tb)] = uin[C][i];
    }
    wave_sync();
    // one store per entry and lane, unconditionally (the address is selected, not the path: a fixed number of stores keeps
    // the waits for the x values requested before them counted); lanes past the last entry repeat its store.  Essential rows
    // never take the direct path when a fix-up is fused (stream_set_essential routes them through the run gather).
#pragma unroll
    for (int r = 0; r < NPL; r++) {
      const int m = (16 * r + 15 < PP) ? t + 16 * r : min(t + 16 * r, PP - 1), mt = m & 15, mr = m >> 4;
      const unsigned fl = (unsigned)side[2 * ((PP + 1) / 2) + 16 * NPK + mt] >> (2 * mr);
      const double v = sm[((unsigned)side[2 * ((PP + 1) / 2) + 16 * (mr >> 2) + mt] >> (8 * (mr & 3))) & 255u];
      const int sv = side[m], df = sv >= 0 ? sv : -1 - sv, d = df & (kExclBit - 1);
      double *yd = a.y;
      if (SPLIT) yd = d < a.nsplit ? a.y : a.yg;
      double *dst = (fl & 2u) ? yd + d : a.ye + ((size_t)e * PP + m);
      *dst = (fl & 1u) ? -v : v;
    }
    wave_sync();  // the LDS strip is reused by the next batch
    if (!more) break;
    b = bn;
#pragma unroll
    for (int r = 0; r < NPL; r++) sA[r] = sB[r], xv[r] = xB[r];
#pragma unroll
    for (int k = 0; k <= NPK; k++) pA[k] = pB[k];
  }
}

// ---- host side ----------------------------------------------------------------------------------------------------------
// Opt-in (PALACE_AMD_STREAM3=1, read at every operator creation, not cached: tests build both forms in one process).  A block
// whose tables exist keeps its form whatever the environment says later (the fused-step query, the split-vector apply).
bool nd_hex_stream3_ok(const SubOp &so) {
  if (so.fe_type != PA_FE_HCURL || so.q1d != 3 || so.p > 2 || !so.qd || !so.d_ye || !so.d_perm_x) return false;
  if (!so.d_idxc && !(getenv("PALACE_AMD_STREAM3") && atoi(getenv("PALACE_AMD_STREAM3")) == 1)) return false;
  return stream_qdata_ok(so);
}

template <int P1, bool U, bool C, bool METRIC, int MINW, bool SPLIT>
static void launch3_kernel(const SubOp &so, NDStream3Args<P1> &a, hipStream_t s) {
  using L = NDLayout<P1, 3>;
  for (int i = 0; i < HalfTab<P1, 3>::LEN; i++) a.tab.Bo[i] = so.Bo[i];
  for (int i = 0; i < HalfTab<P1 + 1, 3>::LEN; i++) a.tab.Bc[i] = so.Bc[i], a.tab.Gc[i] = so.Gc[i];
  constexpr int PP = 3 * P1 * (P1 + 1) * (P1 + 1), NPK = ((PP + 15) / 16 + 3) / 4;
  const size_t lds = sizeof(double) * (size_t)(kWavesPerBlock * 4) * stream3_lds_elem(L::ELEM_PAD + (PP + 1) / 2 + (NPK + 1) * 8 + 12);
  const int wg_env = stream_env_int("PALACE_AMD_STREAM_WG");
  // workgroups per CU: what the registers and the LDS admit, and not more than the occupancy query says
  static const int per_cu_query =
      std::min({stream_occupancy(nd_hex_stream3_kernel<P1, U, C, METRIC, MINW, SPLIT>, 64 * kWavesPerBlock, lds, MINW * 4 / kWavesPerBlock),
                (int)(160 * 1024 / lds), 8});
  a.nbatch = (so.ne + 3) / 4;
  if (a.nbatch == 0) return;
  a.chunk = (a.nbatch + 7) / 8;
  const int wgx = stream_wgx(wg_env > 0 ? wg_env : per_cu_query, a.chunk, kWavesPerBlock, true);
  hipLaunchKernelGGL((nd_hex_stream3_kernel<P1, U, C, METRIC, MINW, SPLIT>), dim3(8 * wgx), dim3(64 * kWavesPerBlock), lds, s, a);
  PA_HIP(hipGetLastError());
}

template <int P1, bool U, bool C, bool METRIC, int MINW>
static void launch3_variant(const SubOp &so, NDStream3Args<P1> &a, hipStream_t s) {
  if (a.nsplit >= 0)  // split vectors (one more instantiation per operator kind)
    return launch3_kernel<P1, U, C, METRIC, MINW, true>(so, a, s);
  launch3_kernel<P1, U, C, METRIC, MINW, false>(so, a, s);
}

template <int P1>
static void launch3_p(const SubOp &so, const double *x, double *y, StreamForm form, hipStream_t s, const SplitIO *split) {
  NDStream3Args<P1> a{};
  stream_set_split(a, split, so.lsize);
  a.ne = so.ne, a.nbatch = 0;
  a.idxc = so.d_idxc;
  a.flagw = so.stream[form].d_flags;
  a.slots = so.d_slots;
  PA_REQUIRE(a.idxc && a.flagw && a.slots, "the streaming tables of this block have not been built");
  a.qdata = so.qd->d;
  a.coef = so.d_coef_s;
  a.x = x, a.y = y, a.ye = so.d_ye;
  const bool m = so.qd->metric;
  PA_REQUIRE(!m || a.coef, "element coefficients of the metric form missing");
  // waves per SIMD the kernels are compiled for (profiles/r13_stream3_resources.txt): four where 128 registers hold the kernel,
  // three for curl-curl + mass (compiled for four, the metric form spills 25 - 40 registers to scratch memory)
  switch (so.qf) {
    case PA_QF_HDIV_33:
      if (m) launch3_variant<P1, false, true, true, 4>(so, a, s); else launch3_variant<P1, false, true, false, 4>(so, a, s);
      break;
    case PA_QF_HCURL_33:
      if (m) launch3_variant<P1, true, false, true, 4>(so, a, s); else launch3_variant<P1, true, false, false, 4>(so, a, s);
      break;
    case PA_QF_HDIVMASS_33:
      // (packed D of both terms, anisotropic materials: twelve rows per point, 36 doubles of q-data per lane)
      if (m) launch3_variant<P1, true, true, true, 3>(so, a, s); else launch3_variant<P1, true, true, false, 3>(so, a, s);
      break;
    default: throw Error("QFunction not available for H(curl) hexahedra");
  }
}

void launch_nd_hex_stream3(const SubOp &so, const double *x, double *y, StreamForm form, hipStream_t s, const SplitIO *split) {
  switch (so.p) {
    case 1: launch3_p<1>(so, x, y, form, s, split); break;
    case 2: launch3_p<2>(so, x, y, form, s, split); break;
    default: throw Error("no three-point streaming H(curl) hex kernel for this order");
  }
}

}  // namespace pa
