// sac_plan.h -- the host-side planner of sac_engine.hip (host code only; included
// after the kernel headers).  plan() at the end is the sequence of steps; the
// decision that matters, which kernels run phases A and C, is choose_path()
// (as a table: DESIGN.md §3.4).
#pragma once

// The kernel family of phases A and C: exactly one per engine.
enum sac_path {
  PATH_SPLIT,  // hidden-split role kernels (sac_split.h)
  PATH_ROLES,  // per-network role kernels (sac_phases.h, ROLES = true)
  PATH_PAIRS,  // pair-tile kernels (sac_pairs.h)
  PATH_ROWS,   // one workgroup per row tile (sac_phases.h, ROLES = false)
  PATH_WIDE,   // layer-synchronous stage path (sac_wide.h)
};

// Launch kinds of a step: A B C D.
enum LaunchKind { L_A = 0, L_B = 1, L_C = 2, L_D = 3 };
struct PhaseLaunch {
  unsigned grid, threads;
  size_t lds;
};

// Workspace offsets of the large-batch stage path (sac_wide.h), from layout_workspace()
struct WideLay {
  int Brw = 0, hp = 0, hq = 0;
  size_t o_dev = 0, o_jobs = 0;
  size_t o_xpi0 = 0, o_xq0 = 0, o_xqt0 = 0, o_xc0 = 0, o_r = 0, o_d = 0, o_lp2 = 0, o_piop = 0;
  size_t o_outpi = 0, o_outq[2] = {0, 0}, o_outqt[2] = {0, 0}, o_outc[2] = {0, 0}, o_da[2] = {0, 0};
  size_t o_P[5][SAC_DEV_LAYERS] = {};      // phase A pre-activations (pi on [s'; s], Q1, Q2, Q1t, Q2t)
  size_t o_Pc[2][SAC_DEV_LAYERS] = {};     // phase C critics
  size_t o_DYq[2][SAC_DEV_LAYERS] = {}, o_DYc[2][SAC_DEV_LAYERS] = {}, o_DYpi[SAC_DEV_LAYERS] = {};
};
#define WIDE_MAX_JOBS 64

struct sac_engine {
  sac_engine_config cfg;
  sac_engine_buffers buf;
  sac_path path = PATH_ROWS;
  PhaseLaunch launch[4] = {};  // by LaunchKind; A and C unused on the stage path (wst)
  EngineDev h;            // host mirror of the device struct
  EngineDev* d = nullptr; // in workspace
  TileDesc* tilesB = nullptr;
  TileDesc* tilesD = nullptr;
  std::vector<TileDesc> hostB, hostD;
  int nB = 0, nD = 0;
  size_t lds_bytes = 0;
  size_t upd_lds = 0;  // dynamic LDS of an update tile (SAC_UPD_LDS_FOR(upd_slots))
  int ncu = 256;  // compute units of the device
  // large-batch stage path (sac_wide.h): layout offsets, stages, jobs
  WideLay wl;
  WideDev wdh;
  WideDev* wdd = nullptr;
  WJob* wjobs = nullptr;
  std::vector<WJob> hostW;
  struct WStage {
    int kind;   // 0 gather, 1 GEMM jobs [j0, j1), 2 pi heads, 3 phase B, 4 phase D
    int j0, j1, grid, phase, last;  // grid: workgroups
    size_t lds;
  };
  std::vector<WStage> wst;
  // graph cache
  hipGraphExec_t gexec = nullptr;
  hipGraph_t graph = nullptr;
  int gchunk = 0;
  sac_replay gkey{};
  hipStream_t cap = nullptr;
  // loop-graph cache (sac_engine_loop_graph): its own graph, exec and key
  struct LoopKey {
    sac_envs envs;
    sac_replay rb;
    int64_t* cursor;
    int32_t done_mode;
    int32_t action_source;
    float* q_ring;
    int32_t q_ring_steps;
    std::vector<int32_t> grad;  // gradient steps after each rollout: its size is k_steps
  };
  hipGraphExec_t lgexec = nullptr;
  hipGraph_t lgraph = nullptr;
  LoopKey lkey{};
  // what the rollout step stores as done (enum sac_done_mode; sac_engine_set_done_mode): host state, read per call
  int32_t done_mode = 0;
  // where a sampled rollout step's actions come from (enum sac_action_source; sac_engine_set_action_source): likewise
  int32_t action_source = 0;
};

static inline int rup(int x, int m) { return (x + m - 1) / m * m; }

struct Layout {
  size_t off = 0;
  size_t take(size_t bytes) {
    off = (off + 255) & ~(size_t)255;
    const size_t o = off;
    off += bytes;
    return o;
  }
};

// ============================================================================ shape
struct NetShape {
  int esz;  // bytes of a GEMM operand element
  // Br: rows of the per-row stashes, whole pairs of row tiles (the pair-tile kernels write 2R rows)
  int B, Bp, nrt, Br, O, A;
  int maxKp, maxNo;  // widest padded hidden / input operand, widest padded output
  NetDev net[5];     // L and every layer's K, N, Kp, Np, w_off, b_off; all else zero
};

static NetShape net_shape(const sac_engine_config* c) {
  NetShape s;
  memset(&s, 0, sizeof(s));
  s.esz = c->precision == SAC_PREC_BF16 ? 2 : 4;
  s.B = c->batch;
  s.Bp = rup(s.B, 32);
  s.nrt = (s.B + SAC_ROWS - 1) / SAC_ROWS;
  s.Br = rup(s.nrt, 2) * SAC_ROWS;
  s.O = c->obs_dim;
  s.A = c->act_dim;
  s.maxKp = s.maxNo = 32;
  for (int ni = 0; ni < 5; ++ni) {
    const bool is_pi = ni == NET_PI;
    const int* dims = is_pi ? c->pi_dims : c->q_dims;
    NetDev& n = s.net[ni];
    n.L = is_pi ? c->pi_layers : c->q_layers;
    int off = 0;
    for (int l = 0; l < n.L; ++l) {
      LayerDev& ly = n.l[l];
      ly.K = dims[l];
      ly.N = dims[l + 1];
      ly.Kp = rup(ly.K, SAC_PAD);
      ly.Np = rup(ly.N, SAC_PAD);
      ly.w_off = off;
      off += ly.K * ly.N;
      ly.b_off = off;
      off += ly.N;
      s.maxKp = std::max(s.maxKp, ly.Kp);
      if (l < n.L - 1) s.maxKp = std::max(s.maxKp, ly.Np);
      else s.maxNo = std::max(s.maxNo, ly.Np);
    }
  }
  return s;
}

// ============================================================================ LDS layout
// LDS layout (floats) of the row-tile / role / pair-tile kernels (policy_act
// included); returns its size and, with hh != null, writes the offsets.
// xrows: rows of the MLP operand buffers (R with roles, 2R where pi runs on
// [s'; s]); full: with pre-activation buffers (the stage path launches none of
// these kernels but policy_act: none); pairs: the pair-tile kernels (sac_pairs.h):
// every per-row buffer 2R rows, pre-activations for one critic or pi at a time
// (no P2 / second outputs); with_red: the hidden split's reduction buffer.
static int lds_layout(const NetShape& s, int xrows, bool full, bool pairs, bool with_red, EngineDev* hh) {
  EngineDev scratch;  // offsets nobody reads
  EngineDev& h = hh ? *hh : scratch;
  const int R = pairs ? 2 * SAC_ROWS : SAC_ROWS, O = s.O, A = s.A;
  h.ld = s.maxKp + 4;
  h.ldo = s.maxNo + 4;
  int lo = 0;
  auto lt = [&](int floats) {
    lo = (lo + 3) & ~3;  // 16-B alignment
    const int o = lo;
    lo += floats;
    return o;
  };
  h.o_X = lt(xrows * h.ld);
  h.o_Y = lt(xrows * h.ld);
  const int Lhq = s.net[NET_Q1].L - 1, Lhp = s.net[NET_PI].L - 1;
  for (int l = 0; full && l < std::max(Lhq, Lhp); ++l) {
    int np = 0;
    if (l < Lhq) np = std::max(np, s.net[NET_Q1].l[l].Np);
    if (l < Lhp) np = std::max(np, s.net[NET_PI].l[l].Np);
    h.ldp1[l] = np + 4;
    h.o_P1[l] = lt(R * h.ldp1[l]);
  }
  for (int l = 0; full && !pairs && l < Lhq; ++l) {
    h.ldp2[l] = s.net[NET_Q2].l[l].Np + 4;
    h.o_P2[l] = lt(R * h.ldp2[l]);
  }
  h.o_s = lt(R * O);
  h.o_s2 = lt(R * O);
  h.o_a = lt(R * A);
  h.o_a2 = lt(R * A);
  h.o_r = lt(R);
  h.o_d = lt(R);
  h.o_et = lt(R * A);
  h.o_ea = lt(R * A);
  h.o_out = lt(xrows * h.ldo);
  h.o_outp = lt(xrows * h.ldo);
  h.o_out2 = pairs ? 0 : lt(R * h.ldo);
  h.o_outp2 = pairs ? 0 : lt(R * h.ldo);
  h.o_lp = lt(R);
  h.o_qt = lt(2 * R);
  h.o_y = lt(R);
  h.o_g = lt(pairs ? 2 * R : R * h.ldo);
  h.o_g2 = pairs ? 0 : lt(R * h.ldo);
  h.o_ga = lt(R * A);
  h.o_gout = lt(R * h.ldo);
  h.o_slot = lt(2 * R);  // int64[R]
  h.o_red = with_red ? lt(SAC_NW * 256) : 0;
  return lo;
}

// Does the phase kernels' layout fit a CU?  (per-network roles: R rows; one
// block per row tile: pi on [s'; s], 2R rows.)  Without the split's reduction
// buffer: the split is decided on the role layout's fit.
struct LdsFits {
  bool roles, rows, pairs;
};
static LdsFits lds_fits(const NetShape& s) {
  auto fits = [&](int xrows, bool pairs) {
    return (size_t)lds_layout(s, xrows, true, pairs, false, nullptr) * 4 <= 160 * 1024;
  };
  return {fits(SAC_ROWS, false), fits(2 * SAC_ROWS, false), fits(2 * SAC_ROWS, true)};
}

// ============================================================================ launch geometry
// Workgroups of phases A and C by path (phase C without its stager blocks).
// Each count is written here once: choose_path tests it against the CUs,
// plan_launches makes it the grid.
#define SAC_PLAN_CUS 256  // co-residency bound of the role kernels' hand-offs: one workgroup per CU
static int split_a_groups(int nrt, int esz) { return nrt * (10 + split_wpi(esz)); }
static int split_c_groups(int nrt, int esz) { return nrt * (2 * split_wcq(esz) + split_wc(esz)); }
static int role_a_groups(int nrt) { return nrt * 6; }
static int role_c_groups(int nrt) { return nrt * 3; }
static int pair_groups(int nrt) { return 2 * ((nrt + 1) / 2); }
static int row_xs(int nrt) {  // largest power of two <= 8 with nrt * xs <= 256 blocks
  int xs = 1;
  while (xs < 8 && nrt * xs * 2 <= SAC_PLAN_CUS) xs *= 2;
  return xs;
}

// ============================================================================ the path
struct PathChoice {
  sac_path path;
  const char* refused;  // an explicit layout override the shape cannot take, else null
};

// Which kernels run phases A and C (DESIGN.md §3.4 has this as a table).
static PathChoice choose_path(const sac_engine_config* c, const NetShape& s, const LdsFits& fits) {
  const int A = s.A, O = s.O, nrt = s.nrt;
  const bool hand_fits = SAC_ROWS * (A + 1) <= SAC_HAND_STRIDE;  // a hand-off payload holds a row tile's actions
  // hidden-split role kernels (sac_split.h): two hidden layers of width 256 in
  // both nets, identity pi output, 2 act <= 32, and every role workgroup of a
  // phase co-resident (phase C: with a stager block per row tile)
  const bool split = c->layout == SAC_LAYOUT_AUTO && fits.roles && c->q_layers == 3 && c->pi_layers == 3 &&
                     c->q_dims[1] == SPLIT_H && c->q_dims[2] == SPLIT_H && c->pi_dims[1] == SPLIT_H &&
                     c->pi_dims[2] == SPLIT_H && c->pi_out_act == SAC_ACT_IDENTITY && 2 * A <= 32 &&
                     split_a_groups(nrt, s.esz) <= SAC_PLAN_CUS &&
                     split_c_groups(nrt, s.esz) + nrt <= SAC_PLAN_CUS && hand_fits;
  // per-network roles: 6 * nrt workgroups must be co-resident (one per CU)
  const bool roles_ok = role_a_groups(nrt) <= SAC_PLAN_CUS && hand_fits && c->layout != SAC_LAYOUT_ROWS &&
                        c->layout != SAC_LAYOUT_PAIRS;
  // Layer-synchronous stage path (sac_wide.h): where the phase
  // kernels' LDS layout does not fit a CU (hidden layers wider than 256, wide
  // inputs: the stage path takes any width), for nets with at least two hidden
  // layers.  At C3 the row-tile kernels are faster (profiles/r04_ab_c3_paths.txt),
  // so they keep the batches they fit; config.stage_path = 1 forces the stage
  // path on any batch past the hidden split, -1 refuses it.
  const bool too_big = !(roles_ok ? fits.roles : fits.rows);
  const bool able = !split && c->q_layers >= 3 && c->pi_layers >= 3 && 2 * A <= WJMAX;
  const bool wide = c->stage_path > 0 ? able : c->stage_path < 0 ? false : able && too_big;
  // pair-tile kernels (sac_pairs.h): two row tiles and one group of networks per
  // workgroup; the critics' seeds are applied by phase B (TileDesc::seed).  The
  // default past the role split wherever its LDS layout fits: C3 4.66K -> 4.90K
  // steps/s fp32, 8.26K -> 9.58K bf16 (profiles/r05_ab_pair_tiles_c3.txt)
  const bool pairs = (c->layout == SAC_LAYOUT_PAIRS || c->layout == SAC_LAYOUT_AUTO) && fits.pairs && hand_fits &&
                     SAC_ROWS * (2 * O + A + 2) <= 4 * SAC_THREADS;  // pair_batch: a record in 4 loads per thread
  const sac_path path = split ? PATH_SPLIT : wide ? PATH_WIDE : roles_ok ? PATH_ROLES : pairs ? PATH_PAIRS : PATH_ROWS;
  // an explicit layout override runs the kernels it names or fails (as stage_path = -1 does)
  const char* refused = nullptr;
  if (c->layout == SAC_LAYOUT_ROLES && path != PATH_ROLES)
    refused = role_a_groups(nrt) > SAC_PLAN_CUS ? "roles (needs 6 * row tiles <= 256 co-resident workgroups)"
              : !hand_fits                      ? "roles (a row tile's actions do not fit the hand-off payload)"
              : too_big                         ? "roles (the R-row LDS layout does not fit: stage path)"
                                                : "roles (stage_path = 1 selects the stage path)";
  if (c->layout == SAC_LAYOUT_PAIRS && path != PATH_PAIRS)
    refused = "pairs (the pair-tile LDS layout or record does not fit)";
  if (c->layout == SAC_LAYOUT_ROWS && path != PATH_ROWS) refused = "rows (the row-tile LDS layout does not fit: stage path)";
  return {path, refused};
}

// ============================================================================ update-tile parts
// Batch parts of an update tile (TileDesc.kpart): the hidden split's layer 0
// reduces over its parts' columns (critics 2: phase A halves; pi wc: phase C
// parts); a large batch (Bp > 1024) is split into P <= 4 parts per phase, P
// chosen for the fewest block rounds x the longest block: a block takes about
// 2 us + its operand bytes at ~25 GB/s (one workgroup per CU; measured on C3:
// 1024 fp32 columns = 256 KB of dY^T / X^T in ~12 us), so at C3 (160 critic
// tiles, 80 policy tiles) P = 3: 480 blocks (2 rounds) for B and 240 (one) for D.
// fp32 hidden-split layer 0: the parts' partial dY summed while staging in one
// block (TileDesc.gsum), which also sees every batch column of the tile -- the
// seeded bias sums of TileDesc.seed rely on that; bf16: a block per dY part
// with a granule hand-off to part 1
// fp32 split layer 0 (wc / 2 summed dY parts: the longest tiles of phases D /
// B, 5 / 3 operand row sets) is also split into 2 batch parts with a granule
// hand-off (the critics' producer parts also hand over their seeded bias
// sums): measured D 8.3 -> 7.6 us on C2.  bf16: the parts' bf16 dY added in
// fp32 and rounded once while staging, one block per tile (23.1K -> 23.6K
// steps/s on C2, B 7.0 -> 6.6, D 6.7 -> 6.2 us, profiles/r04_ab_gsum_bf16_c2.txt)
#define SAC_UPD_TS 32  // update tiles are 32 x 32 weight blocks (64 x 64 measured slower at C3: profiles/r04_ab_tile64_c3.txt)
// the 32 x 32 tiles sum the bias gradient from their staged dY rows (16-B
// LDS reads) instead of loading per-row-tile partials (at C3 256 strided
// loads per column made the k0 == 0 tiles the tail of phases B and D): C3
// 4.47K -> 4.57K fp32, 7.63K -> 8.0K bf16; C2 19.3K -> 19.5K fp32, 23.45K ->
// 24.0K bf16 (profiles/r04_ab_bias_staged.txt)
struct UpdParts {
  int B, D;        // batch parts of the critics' (phase B) and the policy's (phase D) tiles
  int l0;          // of the hidden split's layer 0, pi's and the critics' alike (0 off the split)
  int of(int ni, int l) const { return l == 0 && l0 ? l0 : ni == NET_PI ? D : B; }
};
static int ntiles_of(const LayerDev& ly) {
  return ((ly.Np + SAC_UPD_TS - 1) / SAC_UPD_TS) * ((ly.Kp + SAC_UPD_TS - 1) / SAC_UPD_TS);
}
static UpdParts update_parts(const sac_engine_config* c, const NetShape& s, bool split) {
  const int Bp = s.Bp, esz = s.esz;
  int tilesBD[2] = {0, 0};  // [critics (B), policy (D)]
  for (int ni = NET_PI; ni <= NET_Q2; ++ni)
    for (int l = 0; l < s.net[ni].L; ++l) tilesBD[ni == NET_PI] += ntiles_of(s.net[ni].l[l]);
  auto batch_parts = [&](int ntiles, int extra) {
    if (Bp <= 1024) return 1;
    if (c->upd_parts > 0) return std::min(4, (int)c->upd_parts);
    int best = 4;
    double bc = 1e30;
    for (int P = 2; P <= 4; ++P) {
      const int rounds = (ntiles * P + extra + 255) / 256;
      const double c = rounds * (2.0 + 64.0 * rup((Bp + P - 1) / P, 32) * esz / 25e3);  // us
      if (c < bc - 1e-9) bc = c, best = P;
    }
    return best;
  };
  const int l0 = split ? std::min(esz == 4 ? 2 : 1, Bp / 32) : 0;
  return {batch_parts(tilesBD[0], 0), batch_parts(tilesBD[1], 1), l0};
}

// ============================================================================ workspace
struct WsLayout {
  size_t o_E = 0, o_tB = 0, o_tD = 0, o_part = 0, total = 0;
  int nB = 0, nD = 0;
  UpdParts parts{};
  WideLay wl;
};

static void layout_wide(const NetShape& s, Layout& lay, WideLay& wl) {
  const int Brw = rup(s.B, 64), A = s.A;
  const NetDev& np = s.net[NET_PI];
  const NetDev& nq = s.net[NET_Q1];
  const int hp = np.L - 1, hq = nq.L - 1;
  wl.Brw = Brw;
  wl.hp = hp;
  wl.hq = hq;
  wl.o_dev = lay.take(sizeof(WideDev));
  wl.o_jobs = lay.take(WIDE_MAX_JOBS * sizeof(WJob));
  wl.o_xpi0 = lay.take((size_t)2 * Brw * np.l[0].Kp * 4);
  wl.o_xq0 = lay.take((size_t)Brw * nq.l[0].Kp * 4);
  wl.o_xqt0 = lay.take((size_t)Brw * nq.l[0].Kp * 4);
  wl.o_xc0 = lay.take((size_t)Brw * nq.l[0].Kp * 4);
  wl.o_r = lay.take((size_t)Brw * 4);
  wl.o_d = lay.take((size_t)Brw * 4);
  wl.o_lp2 = lay.take((size_t)Brw * 4);
  wl.o_piop = lay.take((size_t)Brw * 2 * A * 4);
  const int ncb_pi = (np.l[hp - 1].Np + 63) / 64, ncb_q = (nq.l[hq - 1].Np + 63) / 64, ncb_da = (nq.l[0].Np + 63) / 64;
  wl.o_outpi = lay.take((size_t)ncb_pi * 2 * Brw * 2 * A * 4);
  for (int qi = 0; qi < 2; ++qi) {
    wl.o_outq[qi] = lay.take((size_t)ncb_q * Brw * 4);
    wl.o_outqt[qi] = lay.take((size_t)ncb_q * Brw * 4);
    wl.o_outc[qi] = lay.take((size_t)ncb_q * Brw * 4);
    wl.o_da[qi] = lay.take((size_t)ncb_da * Brw * A * 4);
  }
  for (int l = 0; l < hp; ++l) wl.o_P[0][l] = lay.take((size_t)2 * Brw * np.l[l].Np * 4);
  for (int l = 1; l + 1 < hp; ++l) wl.o_DYpi[l] = lay.take((size_t)Brw * np.l[l].Np * 4);
  for (int qi = 0; qi < 2; ++qi) {
    for (int l = 0; l < hq; ++l) {
      const size_t bytes = (size_t)Brw * nq.l[l].Np * 4;
      wl.o_P[1 + qi][l] = lay.take(bytes);
      wl.o_P[3 + qi][l] = lay.take(bytes);
      wl.o_Pc[qi][l] = lay.take(bytes);
    }
    for (int l = 1; l + 1 < hq; ++l) {
      wl.o_DYq[qi][l] = lay.take((size_t)Brw * nq.l[l].Np * 4);
      wl.o_DYc[qi][l] = lay.take((size_t)Brw * nq.l[l].Np * 4);
    }
  }
}

// Every workspace offset; the networks' shapes and (with base != null) their
// workspace pointers go into h.  The sizing call passes base = null.
static WsLayout layout_workspace(const sac_engine_config* c, const NetShape& s, sac_path path, char* base,
                                 EngineDev& h) {
  const int esz = s.esz, Bp = s.Bp, Br = s.Br, nrt = s.nrt, O = s.O, A = s.A;
  const bool split = path == PATH_SPLIT;
  Layout lay;
  WsLayout ws;
  ws.o_E = lay.take(4096);  // EngineDev, padded for prefetch_engine()
  auto P = [&](size_t o) -> void* { return base ? (void*)(base + o) : nullptr; };
  // batch columns of layer 0's operands under the split: X^T 2 Bp (phase A's two
  // halves store it), dY^T 2 Bp for the critics (phase A halves), split_wc Bp for
  // pi (phase C parts)
  const int bp0 = split ? 2 * Bp : Bp;
  const int bp0_pi = split ? split_wc(esz) * Bp : Bp;
  size_t xt_q0 = 0;
  memcpy(h.net, s.net, sizeof(h.net));
  for (int ni = 0; ni < 5; ++ni) {
    const bool is_pi = ni == NET_PI;
    const bool trainable = ni <= NET_Q2;
    NetDev& nd = h.net[ni];
    nd.hid_act = is_pi ? c->pi_hidden_act : c->q_hidden_act;
    nd.out_act = is_pi ? c->pi_out_act : c->q_out_act;
    for (int l = 0; l < nd.L; ++l) {
      LayerDev& ly = nd.l[l];
      ly.Wc = P(lay.take((size_t)ly.Np * ly.Kp * esz));
      if (trainable) {
        const int bpl = l == 0 ? bp0 : Bp;
        ly.WTc = P(lay.take((size_t)ly.Kp * ly.Np * esz));
        if (ni == NET_Q2 && l == 0) {
          ly.XT = P(xt_q0);
        } else {
          // pi: two copies by step parity (from the fused step, where phase D of
          // step k read one while phase A of step k + 1 wrote the other in one
          // launch; with one phase per launch they only alternate)
          const size_t o = lay.take((size_t)ly.Kp * bpl * esz * (is_pi ? 2 : 1));
          if (ni == NET_Q1 && l == 0) xt_q0 = o;
          ly.XT = P(o);
          ly.xt_par = is_pi ? (long)ly.Kp * bpl : 0;
        }
        const int bpg = (l == 0 && is_pi) ? bp0_pi : bpl;
        ly.GT = P(lay.take((size_t)ly.Np * bpg * esz));
        // the update tiles sum the bias gradient from their staged dY^T rows:
        // no per-row-tile partials (TileDesc / store_T with dbp == null)
        ly.dbp = nullptr;
      }
      if (is_pi) ly.pstash = (float*)P(lay.take((size_t)Br * ly.Np * 4));
      if (is_pi) ly.pmask = (uint32_t*)P(lay.take((size_t)Br * ((ly.Np + 31) / 32) * 4));
    }
  }
  h.s_st = (float*)P(lay.take((size_t)Br * O * 4));
  h.a_st = (float*)P(lay.take((size_t)Br * A * 4));
  h.lp_st = (float*)P(lay.take((size_t)2 * Br * 4));
  h.head_st = (float*)P(lay.take((size_t)Br * 4 * A * 4));
  h.lossp = (float*)P(lay.take((size_t)2 * nrt * 4 * 4));
  h.seedq = (float*)P(lay.take((size_t)2 * Bp * 4));
  h.adam_sc = (float*)P(lay.take(2 * 6 * 4));
  h.alpha_sc = (double*)P(lay.take(2 * 2 * 8));
  h.sync = (uint32_t*)P(lay.take((size_t)(SYNC_FLAGS + HK_COUNT * nrt * 16) * 4));
  h.hand = (float*)P(lay.take((size_t)HK_COUNT * nrt * SAC_HAND_STRIDE * 4));
  h.gstride = SAC_ROWS * (A + 1);
  h.gran = (uint64_t*)P(lay.take((size_t)G_COUNT * nrt * h.gstride * 8));
  h.stg_stride = (16 + 2 * SAC_ROWS * O + SAC_ROWS * A + 2 * SAC_ROWS + 15) / 16 * 16;
  h.stg = (float*)P(lay.take((size_t)2 * nrt * h.stg_stride * 4));  // two records per row tile: by step parity
  h.gs2 = SAC_ROWS * std::max(2 * A, A + 1);
  h.gran2 = (uint64_t*)P(lay.take((size_t)GS_COUNT * nrt * SPLIT_GP * h.gs2 * 8));
  if (path == PATH_WIDE) layout_wide(s, lay, ws.wl);
  ws.parts = update_parts(c, s, split);
  int nhalf = 0;
  for (int ni = NET_PI; ni <= NET_Q2; ++ni)
    for (int l = 0; l < s.net[ni].L; ++l) {
      const int t = ntiles_of(s.net[ni].l[l]);
      const int parts = ws.parts.of(ni, l);
      (ni == NET_PI ? ws.nD : ws.nB) += t * parts;
      nhalf += t * (parts - 1);  // producer parts: one granule slot each
    }
  ws.o_tB = lay.take((size_t)ws.nB * sizeof(TileDesc));
  ws.o_tD = lay.take((size_t)ws.nD * sizeof(TileDesc));
  ws.o_part = lay.take((size_t)nhalf * SAC_PART_STRIDE * 8);  // batch-part partial dW granules
  ws.total = lay.take(0);
  return ws;
}

// ============================================================================ device descriptor
// The scalars, hyper-parameters and parameter buffers of the device descriptor
// (the networks and workspace pointers are layout_workspace's).
static void fill_engine_dev(const sac_engine_config* c, const NetShape& s, sac_path path,
                            const sac_engine_buffers& buf, EngineDev& h) {
  h.B = s.B;
  h.Bp = s.Bp;
  h.Br = s.Br;
  h.O = s.O;
  h.A = s.A;
  h.nrt = s.nrt;
  h.xs = row_xs(s.nrt);
  // the kernels' view of the path, assigned here only.  The hidden-split kernels
  // are role kernels: roles is set under the split too.
  h.split = path == PATH_SPLIT;
  h.roles = path == PATH_SPLIT || path == PATH_ROLES;
  h.pairs = path == PATH_PAIRS;
  // phase A's weight parts on one or two XCDs each: A's fetched bytes 11.0 -> 5.1
  // MB per launch, phase B 8.6 -> 8.1 us, +1.2% steps/s (C2 fp32,
  // profiles/r03_ab_role_xcd.txt)
  h.role_xcd = path == PATH_SPLIT && split_a_groups(s.nrt, s.esz) % 8 == 0;
  // phase C stages the next step's batch (config.stage_batch = -1 turns it off)
  h.stage = c->stage_batch >= 0;
  h.auto_entropy = c->auto_entropy;
  h.alpha_update = 1;
  h.gamma = c->gamma;
  h.tau = c->tau;
  h.ls_min = c->log_std_min;
  h.ls_max = c->log_std_max;
  h.scale = c->action_scale;
  h.actor_lr = c->actor_lr;
  h.critic_lr = c->critic_lr;
  h.beta1 = c->beta1;
  h.beta2 = c->beta2;
  h.adam_eps = c->adam_eps;
  h.target_entropy = c->target_entropy;
  h.alpha_lr = c->alpha_lr;
  h.seed = c->seed;
  h.spin_limit = 1 << 22;
  float* parts[5] = {buf.pi, buf.q1, buf.q2, buf.q1t, buf.q2t};
  float* ms[3] = {buf.pi_m, buf.q1_m, buf.q2_m};
  float* vs[3] = {buf.pi_v, buf.q1_v, buf.q2_v};
  for (int ni = 0; ni < 5; ++ni) {
    h.net[ni].P = parts[ni];
    h.net[ni].M = ni < 3 ? ms[ni] : nullptr;
    h.net[ni].V = ni < 3 ? vs[ni] : nullptr;
    for (int l = 0; l < h.net[ni].L; ++l) h.net[ni].l[l].bias = parts[ni] + h.net[ni].l[l].b_off;
  }
  h.alpha_state = buf.alpha_state;
  h.opt_steps = buf.opt_steps;
  h.rng_step = buf.rng_step;
  h.stats = buf.stats;
  // update tiles stage up to 2 batch chunks of 512 B per operand row per round
  // (every tile reduces over at most Bp columns: split layer 0 is two half tiles)
  const int bch = 512 / s.esz;
  h.upd_slots = std::min(2, (s.Bp + bch - 1) / bch);
}

// Grid, block and dynamic LDS of the four phase launches (the stage path
// launches B and D from here and A and C from its stage list).
static void plan_launches(sac_engine* e, const NetShape& s) {
  const sac_engine_config* c = &e->cfg;
  const unsigned nrt = s.nrt, stg = e->h.stage ? nrt : 0;  // stager blocks of phase C
  const size_t lf = std::max(e->lds_bytes, e->upd_lds);
  switch (e->path) {
    case PATH_SPLIT:
      e->launch[L_A] = {(unsigned)split_a_groups(nrt, s.esz), SAC_THREADS, lf};
      e->launch[L_C] = {split_c_groups(nrt, s.esz) + stg, SAC_THREADS, lf};
      break;
    case PATH_ROLES:
      e->launch[L_A] = {(unsigned)role_a_groups(nrt), SAC_THREADS, lf};
      e->launch[L_C] = {role_c_groups(nrt) + stg, SAC_THREADS, lf};
      break;
    case PATH_PAIRS:
      e->launch[L_A] = {(unsigned)pair_groups(nrt), SAC_THREADS, lf};
      e->launch[L_C] = {pair_groups(nrt) + stg, SAC_THREADS, lf};
      break;
    case PATH_ROWS:
      e->launch[L_A] = {nrt * e->h.xs, SAC_THREADS, lf};
      e->launch[L_C] = {nrt * e->h.xs + stg, SAC_THREADS, lf};
      break;
    case PATH_WIDE:
      break;
  }
  // phase B in 2 rounds of 1024-thread blocks (C3: 480 blocks) -> 512-thread
  // blocks with 2 slots, two per CU, one round: C3 B 37.0 -> 33.5 us fp32,
  // 20.0 -> 18.1 bf16 (profiles/r04_ab_upd_ut512_c3.txt); config.upd_threads =
  // 512 / 1024 forces it (no summed layer-0 tiles: GS 1 only, so never with the
  // hidden split)
  bool ut512 = e->nB > 256 && e->nB <= 512;
  if (c->upd_threads) ut512 = c->upd_threads == 512;
  if (ut512 && e->path != PATH_SPLIT)
    e->launch[L_B] = {(unsigned)e->nB, 512, SAC_UPD_LDS_FOR(1)};  // one slot (sac_phases.h, dw_adam_tile)
  else
    e->launch[L_B] = {(unsigned)e->nB, SAC_UPD_THREADS, e->upd_lds};
  e->launch[L_D] = {(unsigned)e->nD + 1, SAC_UPD_THREADS, e->upd_lds};
}

// ============================================================================ update tiles
// Update-tile order for the XCDs (speed only; any order gives the same bits).
// Blocks are dealt round-robin to the 8 XCDs (block b on XCD b % 8), and the
// dW operands come from other XCDs' L2s (fetched through the Infinity Fabric
// at ~11 B/cycle per CU). A layer's tile (nt, kt) reads dY^T rows nt and X^T
// rows kt; tiles sharing them on one XCD fetch them once into that L2. So each
// net's tiles are bucketed by XCD -- a 256x256 layer's 8x8 tiles as 2 nt x 4 kt
// blocks per XCD (6 row groups fetched per XCD instead of 16), one-column /
// one-row layers dealt across the XCDs -- and emitted so that position p holds
// a tile of bucket p % 8.
static void xcd_order(std::vector<TileDesc>& tiles) {
  std::vector<TileDesc> out;
  out.reserve(tiles.size());
  size_t i = 0;
  while (i < tiles.size()) {
    size_t j = i;  // one net: consecutive tiles of the same optimizer
    while (j < tiles.size() && tiles[j].opt == tiles[i].opt) ++j;
    std::vector<TileDesc> bucket[8];
    for (size_t t = i; t < j; ++t) {
      const TileDesc& d = tiles[t];
      const int NT = d.Np / 32, KT = d.Kp / 32, nt = d.n0 / 32, kt = d.k0 / 32;
      int x;
      if (KT == 1) x = nt % 8;
      else if (NT == 1) x = kt % 8;
      else if (NT >= 4 && KT >= 2) x = (nt * 4 / NT) * 2 + (kt * 2 / KT);
      else x = (nt * KT + kt) % 8;
      bucket[x].push_back(d);
    }
    size_t taken[8] = {0};
    for (size_t left = j - i; left;) {
      for (int x = 0; x < 8; ++x)
        if (taken[x] < bucket[x].size()) {
          out.push_back(bucket[x][taken[x]++]);
          --left;
        }
    }
    i = j;
  }
  tiles.swap(out);
}

// The consumer tile (nt, kt) of layer l of net ni, whole batch (build_update_tiles parts it).
static TileDesc update_tile(const sac_engine* e, int ni, int l, int nt, int kt) {
  const EngineDev& h = e->h;
  const int TS = SAC_UPD_TS, Bp = h.Bp, esz = e->cfg.precision == SAC_PREC_BF16 ? 2 : 4;
  const bool split = e->path == PATH_SPLIT, pairs = e->path == PATH_PAIRS;
  const int wc = split_wc(esz);
  const NetDev& nd = h.net[ni];
  const NetDev& tn = h.net[ni == NET_PI ? NET_PI : ni + 2];
  const LayerDev& ly = nd.l[l];
  TileDesc t;
  memset(&t, 0, sizeof(t));
  const int bpl = (l == 0 && split) ? 2 * Bp : Bp;                        // X^T row stride
  const int bpg = (l == 0 && split) ? (ni == NET_PI ? wc : 2) * Bp : Bp;  // dY^T row stride
  t.GT = (const char*)ly.GT + (size_t)nt * TS * bpg * esz;
  t.XT = (const char*)ly.XT + (size_t)kt * TS * bpl * esz;
  t.W = nd.P + ly.w_off;
  t.Wm = nd.M + ly.w_off;
  t.Wv = nd.V + ly.w_off;
  t.b = nd.P + ly.b_off;
  t.bm = nd.M + ly.b_off;
  t.bv = nd.V + ly.b_off;
  t.Wc = ly.Wc;
  t.WTc = ly.WTc;
  if (ni != NET_PI) {
    t.tW = tn.P + ly.w_off;
    t.tb = tn.P + ly.b_off;
    t.tWc = tn.l[l].Wc;
  }
  t.xt_par = ly.xt_par;
  t.bp = bpl;
  t.K = ly.K;
  t.N = ly.N;
  t.Kp = ly.Kp;
  t.Np = ly.Np;
  t.n0 = nt * TS;
  t.k0 = kt * TS;
  t.opt = ni;
  t.ld = t.bp;
  t.ldx = t.bp;
  t.kpart = 0;
  t.nparts = 1;
  t.gsum = 1;
  t.goff = 0;
  t.seed = nullptr;
  if ((split || pairs) && ni != NET_PI) t.seed = h.seedq + (size_t)(ni - NET_Q1) * Bp;
  if (l == 0 && split) {  // one block: dY parts [p Bp, (p+1) Bp) summed, X^T [0, Bp)
    t.gsum = ni == NET_PI ? wc : 2;
    t.goff = Bp;
    t.bp = Bp;
    t.ld = bpg;
    t.ldx = 2 * Bp;
  }
  return t;
}

// Self-contained update tiles (phase B: critics + Polyak, phase D: policy) into
// e->hostB / hostD, producer parts first.
static void build_update_tiles(sac_engine* e, const WsLayout& ws, char* base) {
  const EngineDev& h = e->h;
  const int TS = SAC_UPD_TS, Bp = h.Bp, esz = e->cfg.precision == SAC_PREC_BF16 ? 2 : 4;
  const bool split = e->path == PATH_SPLIT;
  e->hostB.clear();
  e->hostD.clear();
  std::vector<TileDesc> halvesB, halvesD;
  int ihalf = 0;
  for (int ni = NET_PI; ni <= NET_Q2; ++ni)
    for (int l = 0; l < h.net[ni].L; ++l) {
      const LayerDev& ly = h.net[ni].l[l];
      for (int nt = 0; nt < (ly.Np + TS - 1) / TS; ++nt)
        for (int kt = 0; kt < (ly.Kp + TS - 1) / TS; ++kt) {
          TileDesc t = update_tile(e, ni, l, nt, kt);
          const int parts = ws.parts.of(ni, l);
          if (parts > 1) {
            // consumer part 1 (batch columns [0, bpp)) + producer parts 2..P ([(p-1) bpp, p bpp));
            // split layer 0 (gsum): batch parts of the summed operands
            const int bpp = rup((Bp + parts - 1) / parts, 32);
            if (!(l == 0 && split)) {
              t.ld = Bp;
              t.ldx = Bp;
            }
            t.bp = bpp;
            t.kpart = 1;
            t.nparts = parts;
            t.part = (uint64_t*)(base + ws.o_part) + (size_t)ihalf * SAC_PART_STRIDE;
            ihalf += parts - 1;
            for (int pp = 2; pp <= parts; ++pp) {
              TileDesc pt = t;
              const int off = (pp - 1) * bpp;
              pt.kpart = pp;
              pt.bp = std::min(bpp, Bp - off);
              pt.GT = (const char*)t.GT + (size_t)off * esz;
              pt.XT = (const char*)t.XT + (size_t)off * esz;
              if (t.seed) pt.seed = t.seed + off;
              (ni == NET_PI ? halvesD : halvesB).push_back(pt);
            }
          }
          (ni == NET_PI ? e->hostD : e->hostB).push_back(t);
        }
    }
  auto order = [&](std::vector<TileDesc>& cons, std::vector<TileDesc>& prod) {
    xcd_order(cons);
    // producer parts first: in-order dispatch starts every producer before its consumer
    cons.insert(cons.begin(), prod.begin(), prod.end());
  };
  order(e->hostB, halvesB);
  order(e->hostD, halvesD);
  e->h.nBq[0] = e->h.nBq[1] = 0;
  for (const TileDesc& t : e->hostB) ++e->h.nBq[t.opt - 1];
}

// ============================================================================ stage path
// A forward GEMM job of the stage path: layer l of net ni on M rows of X.
static WJob wide_fwd_job(const EngineDev& h, int ni, int l, int M, const float* X, float* Pd, void* XT, int xt_row0,
                         long xt_par, float* OUTP, int p_row0 = 0) {
  const NetDev& nd = h.net[ni];
  const LayerDev& ly = nd.l[l];
  WJob j;
  memset(&j, 0, sizeof(j));
  j.M = M;
  j.K = ly.K;
  j.Kp = ly.Kp;
  j.N = ly.N;
  j.Np = ly.Np;
  j.nrb = M / 64;
  j.ncb = (ly.Np + 63) / 64;
  j.amode = l == 0 ? WA_PLAIN : WA_ACT;
  j.aact = nd.hid_act;
  j.X = X;
  j.ldx = ly.Kp;
  j.Wp = ly.Wc;
  j.tcols = ly.Kp;
  j.bias = nd.P + ly.b_off;
  j.emode = WE_FWD;
  j.P = Pd;
  j.p_row0 = p_row0;
  j.ldp = ly.Np;
  j.oact = nd.hid_act;
  j.XT = XT;
  j.xt_row0 = xt_row0;
  j.xt_ld = h.Bp;
  j.xt_par = xt_par;
  if (OUTP) {
    const LayerDev& lo = nd.l[nd.L - 1];
    j.Wout = nd.P + lo.w_off;
    j.ldwout = lo.K;
    j.Nout = lo.N;
    j.OUTP = OUTP;
    j.outp_cb = (long)M * lo.N;
  }
  j.pact = -1;
  return j;
}

// A backward GEMM job through layer d: dX_d = dY_d W_d -> dY_{d-1} = act'(P_{d-1}) dX_d
static WJob wide_bwd_job(const EngineDev& h, int Brw, int ni, int d, int M, const float* X, bool first, int rowpro,
                         int qi, const float* Pprev, float* DY, void* GT, float* dbp, float* DA) {
  const NetDev& nd = h.net[ni];
  const LayerDev& ly = nd.l[d];
  const LayerDev& lb = nd.l[d - 1];
  const LayerDev& lo = nd.l[nd.L - 1];
  WJob j;
  memset(&j, 0, sizeof(j));
  j.M = M;
  j.K = ly.N;
  j.Kp = ly.Np;
  j.N = ly.K;
  j.Np = ly.Kp;
  j.nrb = M / 64;
  j.ncb = (ly.Kp + 63) / 64;
  j.amode = first ? WA_OUTBWD : WA_PLAIN;
  j.aact = nd.hid_act;
  j.X = X;
  j.ldx = ly.Np;
  if (first) {
    j.Wo = nd.P + lo.w_off;
    j.ldwo = lo.K;
    j.J = lo.N;
    j.rowpro = rowpro;
    j.qi = qi;
    if (GT) {  // phase A / pi: the generated dY of layer d is a dW operand too
      j.AGT = ly.GT;
      j.Adbp = ly.dbp;
      j.adbp_ld = ly.N;
    }
  }
  j.Wp = ly.WTc;
  j.tcols = ly.Np;
  j.emode = WE_BWD;
  j.Pprev = Pprev;
  j.ldpp = lb.Np;
  j.pact = nd.hid_act;
  j.DY = DY;
  j.lddy = lb.Np;
  j.GT = GT;
  j.gt_ld = h.Bp;
  j.dbp = dbp;
  j.dbp_ld = lb.N;
  if (DA) {
    const LayerDev& l0 = nd.l[0];
    j.W0a = nd.P + l0.w_off;
    j.ldw0 = l0.K;
    j.a_off = h.O;
    j.DA = DA;
    j.da_cb = (long)Brw * h.A;
  }
  return j;
}

// The stage path's device descriptor (sac_wide.h).
static void fill_wide_dev(sac_engine* e, char* base) {
  const WideLay& wl = e->wl;
  const EngineDev& h = e->h;
  auto F = [&](size_t o) { return (float*)(base + o); };
  WideDev& W = e->wdh;
  memset(&W, 0, sizeof(W));
  const int A = h.A, Brw = wl.Brw, hp = wl.hp, hq = wl.hq;
  const NetDev& np = h.net[NET_PI];
  const NetDev& nq1 = h.net[NET_Q1];
  W.B = h.B;
  W.Bp = h.Bp;
  W.Brw = Brw;
  W.nrt = h.nrt;
  W.O = h.O;
  W.A = A;
  W.ldpi0 = np.l[0].Kp;
  W.ldq0 = nq1.l[0].Kp;
  W.Xpi0 = F(wl.o_xpi0);
  W.Xq0 = F(wl.o_xq0);
  W.Xqt0 = F(wl.o_xqt0);
  W.Xc0 = F(wl.o_xc0);
  W.R = F(wl.o_r);
  W.Dn = F(wl.o_d);
  W.LP2 = F(wl.o_lp2);
  W.PIOP = F(wl.o_piop);
  W.ncb_pi = (np.l[hp - 1].Np + 63) / 64;
  W.ncb_q = (nq1.l[hq - 1].Np + 63) / 64;
  W.ncb_da = (nq1.l[0].Np + 63) / 64;
  W.cbs_pi = (long)2 * Brw * 2 * A;
  W.cbs_q = Brw;
  W.cbs_da = (long)Brw * A;
  W.OUTPpi = F(wl.o_outpi);
  for (int qi = 0; qi < 2; ++qi) {
    W.OUTPq[qi] = F(wl.o_outq[qi]);
    W.OUTPqt[qi] = F(wl.o_outqt[qi]);
    W.OUTPc[qi] = F(wl.o_outc[qi]);
    W.DA[qi] = F(wl.o_da[qi]);
    W.GTq_out[qi] = h.net[NET_Q1 + qi].l[hq].GT;
    W.dbpq_out[qi] = h.net[NET_Q1 + qi].l[hq].dbp;
  }
  W.GTpi_out = np.l[hp].GT;
  W.dbppi_out = np.l[hp].dbp;
  W.rng_step = e->buf.rng_step;
  W.stamp_stage = -1;
#ifdef SAC_STAMPS  // diagnostic build only: the stage that writes stamps (tools/wide_stamps.py)
  if (const char* v = getenv("SAC_WIDE_STAMP_STAGE")) W.stamp_stage = atoi(v);
#endif
  e->wdd = (WideDev*)(base + wl.o_dev);
  e->wjobs = (WJob*)(base + wl.o_jobs);
}

// One GEMM stage of the jobs js: its items, K-block buffers and LDS.
static void add_wide_gemm_stage(sac_engine* e, std::vector<WJob> js, int phase, int last) {
  // the two K-block buffers + the epilogue's weight slices (WWS floats); WA_OUTBWD
  // adds the row seeds and the output layer's weights
  // K-block buffers: as many (2..4) as keep the stage's workgroups co-resident
  // in one round (items / CUs per CU) in 160 KiB of LDS per CU
  const size_t kbuf = e->cfg.precision == SAC_PREC_FP32 ? WK<float>::BUF : WK<bf16>::BUF;  // floats
  const int ncu = e->ncu > 0 ? e->ncu : 256;
  int item = 0;
  size_t extra = WWS;  // floats past the K buffers
  for (WJob& j : js) {
    if (j.amode != js[0].amode) fprintf(stderr, "sac_engine: internal: mixed A modes in one stage\n"), abort();
    j.item0 = item;
    item += j.nrb * j.ncb;
    if (j.amode == WA_OUTBWD) extra = std::max(extra, (size_t)WWS + 64 * WLDD + (size_t)j.J * j.Kp);
    if ((j.OUTP && (size_t)j.Nout * WBN > WWS) || (j.DA && (size_t)WBN * e->h.A > WWS)) extra = ~(size_t)0 / 64;  // refused
  }
  const int per_cu = std::max(1, (item + ncu - 1) / ncu);
  int nb = 2;
  for (int b = 4; b > 2; --b)
    if ((size_t)per_cu * (b * kbuf + extra) * 4 <= 160 * 1024) {
      nb = b;
      break;
    }
  for (WJob& j : js) j.nbuf = nb;
  const size_t lf = nb * kbuf + extra;
  std::vector<WJob>& JB = e->hostW;
  sac_engine::WStage st{1, (int)JB.size(), (int)(JB.size() + js.size()), item, phase, last, lf * 4};
  e->wst.push_back(st);
  JB.insert(JB.end(), js.begin(), js.end());
}

// The large-batch path's device descriptor, jobs and stage list (sac_wide.h):
// per step  gather | A forward stages | pi heads | Qt forward stages | critic
// backward stages | B | C critic forward | critic dX | pi backward | D.
static void build_wide(sac_engine* e, char* base) {
  fill_wide_dev(e, base);
  const WideLay& wl = e->wl;
  const EngineDev& h = e->h;
  const WideDev& W = e->wdh;
  auto F = [&](size_t o) { return (float*)(base + o); };
  const int B = h.B, A = h.A, Brw = wl.Brw, hp = wl.hp, hq = wl.hq;
  const NetDev& np = h.net[NET_PI];
  e->hostW.clear();
  e->wst.clear();
  auto add = [&](int kind, int grid, int phase) {
    sac_engine::WStage st{kind, 0, 0, grid, phase, 0, 0};
    e->wst.push_back(st);
  };
  // ---- phase A
  add(0, (B + WGR - 1) / WGR, 0);  // gather
  for (int d = 0; d < std::max(hp, hq); ++d) {
    std::vector<WJob> js;
    if (d < hp)
      // the last hidden layer's P is read by pi's backward only: actor rows [Brw, 2 Brw)
      js.push_back(wide_fwd_job(h, NET_PI, d, 2 * Brw, d ? F(wl.o_P[0][d - 1]) : W.Xpi0, F(wl.o_P[0][d]),
                                np.l[d + 1].XT, Brw, np.l[d + 1].xt_par, d == hp - 1 ? W.OUTPpi : nullptr,
                                d == hp - 1 ? Brw : 0));
    for (int qi = 0; qi < 2; ++qi)
      if (d < hq)
        js.push_back(wide_fwd_job(h, NET_Q1 + qi, d, Brw, d ? F(wl.o_P[1 + qi][d - 1]) : W.Xq0, F(wl.o_P[1 + qi][d]),
                                  h.net[NET_Q1 + qi].l[d + 1].XT, 0, 0, d == hq - 1 ? W.OUTPq[qi] : nullptr));
    add_wide_gemm_stage(e, js, 0, 0);
  }
  {
    const int AP = A <= 1 ? 1 : 1 << (32 - __builtin_clz(A - 1));
    const int rpb = WG_T / AP;
    add(2, (2 * Brw + rpb - 1) / rpb, 0);  // pi heads
  }
  for (int d = 0; d < hq; ++d) {
    std::vector<WJob> js;
    for (int qi = 0; qi < 2; ++qi)
      js.push_back(wide_fwd_job(h, NET_Q1T + qi, d, Brw, d ? F(wl.o_P[3 + qi][d - 1]) : W.Xqt0,
                                d < hq - 1 ? F(wl.o_P[3 + qi][d]) : nullptr, nullptr, 0, 0,  // no backward: last P unread
                                d == hq - 1 ? W.OUTPqt[qi] : nullptr));
    add_wide_gemm_stage(e, js, 0, 0);
  }
  for (int d = hq - 1; d >= 1; --d) {
    std::vector<WJob> js;
    for (int qi = 0; qi < 2; ++qi) {
      const NetDev& nq = h.net[NET_Q1 + qi];
      const bool first = d == hq - 1;
      js.push_back(wide_bwd_job(h, Brw, NET_Q1 + qi, d, Brw, first ? F(wl.o_P[1 + qi][d]) : F(wl.o_DYq[qi][d]), first,
                                WR_YSEED, qi, F(wl.o_P[1 + qi][d - 1]), d - 1 >= 1 ? F(wl.o_DYq[qi][d - 1]) : nullptr,
                                nq.l[d - 1].GT, nq.l[d - 1].dbp, nullptr));
    }
    add_wide_gemm_stage(e, js, 0, 0);
  }
  add(3, 0, 1);  // phase B
  // ---- phase C
  for (int d = 0; d < hq; ++d) {
    std::vector<WJob> js;
    for (int qi = 0; qi < 2; ++qi)
      js.push_back(wide_fwd_job(h, NET_Q1 + qi, d, Brw, d ? F(wl.o_Pc[qi][d - 1]) : W.Xc0, F(wl.o_Pc[qi][d]), nullptr,
                                0, 0, d == hq - 1 ? W.OUTPc[qi] : nullptr));
    add_wide_gemm_stage(e, js, 2, 0);
  }
  for (int d = hq - 1; d >= 1; --d) {
    std::vector<WJob> js;
    for (int qi = 0; qi < 2; ++qi) {
      const bool first = d == hq - 1;
      js.push_back(wide_bwd_job(h, Brw, NET_Q1 + qi, d, Brw, first ? F(wl.o_Pc[qi][d]) : F(wl.o_DYc[qi][d]), first,
                                WR_MINQ, qi, F(wl.o_Pc[qi][d - 1]), d - 1 >= 1 ? F(wl.o_DYc[qi][d - 1]) : nullptr,
                                nullptr, nullptr, d == 1 ? W.DA[qi] : nullptr));
    }
    add_wide_gemm_stage(e, js, 2, 0);
  }
  for (int d = hp - 1; d >= 1; --d) {
    const bool first = d == hp - 1;
    std::vector<WJob> js;
    js.push_back(wide_bwd_job(h, Brw, NET_PI, d, Brw,
                              first ? F(wl.o_P[0][d]) + (size_t)Brw * np.l[d].Np : F(wl.o_DYpi[d]), first, WR_PIHEAD, 0,
                              F(wl.o_P[0][d - 1]) + (size_t)Brw * np.l[d - 1].Np,
                              d - 1 >= 1 ? F(wl.o_DYpi[d - 1]) : nullptr, np.l[d - 1].GT, np.l[d - 1].dbp, nullptr));
    add_wide_gemm_stage(e, js, 2, d == 1);
  }
  add(4, 0, 3);  // phase D
}

// ============================================================================ plan
struct PlanSize {
  size_t bytes;         // of workspace
  const char* refused;  // choose_path's: create fails on it, the workspace query ignores it
};

// Lays out everything; when e != nullptr also fills the engine (base = workspace).
static PlanSize plan(const sac_engine_config* c, sac_engine* e, char* base) {
  const NetShape s = net_shape(c);
  const PathChoice pc = choose_path(c, s, lds_fits(s));
  EngineDev h;
  memset(&h, 0, sizeof(h));
  const WsLayout ws = layout_workspace(c, s, pc.path, base, h);
  if (e) {
    // the one-block-per-row-tile kernels run pi on [s'; s] (2R rows); with roles
    // every MLP pass is R rows
    const bool pairs = pc.path == PATH_PAIRS, wide = pc.path == PATH_WIDE;
    const bool r_rows = wide || pc.path == PATH_ROLES || pc.path == PATH_SPLIT;
    const int lo = lds_layout(s, r_rows ? SAC_ROWS : 2 * SAC_ROWS, !wide, pairs, pc.path == PATH_SPLIT, &h);
    fill_engine_dev(c, s, pc.path, e->buf, h);
    e->d = (EngineDev*)(base + ws.o_E);
    h.tilesB = e->tilesB = (TileDesc*)(base + ws.o_tB);
    h.tilesD = e->tilesD = (TileDesc*)(base + ws.o_tD);
    e->nB = h.nB = ws.nB;
    e->nD = h.nD = ws.nD;
    memcpy(&e->h, &h, sizeof(h));  // padding included: sac_debug_plan_host hashes the bytes
    e->path = pc.path;
    e->lds_bytes = (size_t)lo * 4;
    e->upd_lds = SAC_UPD_LDS_FOR(h.upd_slots);
    e->wl = ws.wl;
    plan_launches(e, s);
    build_update_tiles(e, ws, base);
    if (wide) build_wide(e, base);
  }
  return {ws.total + 256, pc.refused};
}
