// lipmpc_solve_ops.inc -- the row operators of one problem (G x, G^T w, K = 2I + G^T D G), the square-root-free factorisation and the two substitutions
// A SECTION OF THE BODY of step_solve (lipmpc_solve.hpp), included there: it shares that function's locals -- the lane
// constants, the row operators, the iterate -- and is no translation unit of its own.
  // ---- linear row maps -------------------------------------------------------------------------
  // rows(x): lin[R_RU] = rr.(x_a - x_{a-1}); lin[R_VU] = wv.v_a(x); lin[R_CBF+t] = eta_t . x_a
  auto rows_lin = [&](double x, double& r_lin, double& w_lin, double (&h_lin)[NOBS_R > 0 ? NOBS_R : 1], double& xx,
                      double& xy) {
    const double xp = gxor<G, 1>(x);
    if constexpr (STREAM) { xx = c ? xp : x; xy = c ? x : xp; }      // streamed rows take (x, y) of the stage
    const double dxo = x - gup<G, 2>(x, lane);                        // own coordinate of p_{a+1} - p_a (p_0 is in r_c)
    r_lin = fma(rq, gxor<G, 1>(dxo), ro * dxo);
    const double ps = prefix_excl2<G>(sgn_a * x, lane);
    const double vl = kap * x + 2.0 * kap * sgn_a * ps;
    w_lin = fma(wq, gxor<G, 1>(vl), wo * vl);
#pragma unroll
    for (int t = 0; t < NOBS_R; ++t) h_lin[t] = fma(oq[t], xp, oo[t] * x);
  };
  // (G^T w)_lane from direction weights: tr (reach dir), tv (velocity dir), wc[t] (LDCBF rows, g = -eta)
  // (axs, ays): sum_t eta_t w_t over this lane's streamed rows
  // (axs, ays): sum_t eta_t w_t over this lane's streamed rows, (x, y) order
  auto GT_apply = [&](double tr, double tv, const double (&wc)[NOBS_R > 0 ? NOBS_R : 1], double axs, double ays) -> double {
    const double reach_own = fma(-rq, gxor<G, 1>(tr), ro * tr);
    double res = reach_own - gdown<G, 2>(reach_own, lane);          // lanes past the last stage hold zeros
    const double uu = fma(-wq, gxor<G, 1>(tv), wo * tv);
    const double suf = suffix_excl2<G>(sgn_a * uu, lane);
    res = fma(kap_l, uu, res);
    res = fma(2.0 * kap_l * sgn_a, suf, res);
    double aown = 0.0, apart = 0.0;                                   // eta-weighted sums for own / partner coordinate
    if constexpr (STREAM) { aown = c ? ays : axs; apart = c ? axs : ays; }
#pragma unroll
    for (int t = 0; t < NOBS_R; ++t) { aown = fma(oo[t], wc[t], aown); apart = fma(oq[t], wc[t], apart); }
    return res - (aown + gxor<G, 1>(apart));
  };

  // ---- K = 2I + G^T D G (lane = row), square-root-free factorisation, solves -----------------------
  double Krow[NV];
  double eqm[NMAX];                      // eqm[b] = 1 if this lane's stage is b
#pragma unroll
  for (int b = 0; b < NMAX; ++b) eqm[b] = (b == a) ? 1.0 : 0.0;
  // dr = d_RU + d_RL, dv = d_VU + d_VL (+ d_M), dc[t] = LDCBF row weights
  // (cxs, cxys, cys): sum_t d_t eta_t eta_t^T over this lane's streamed rows
  auto form_K = [&](double dr, double dv, const double (&dc)[NOBS_R > 0 ? NOBS_R : 1], double cxs, double cxys, double cys) {
    const double drp = gxor<G, 1>(dr);
    const double d0 = c ? drp : dr, d1 = c ? dr : drp;
    // F = Rr^T diag(d0,d1) Rr, Rr = [[cr,sr],[-sr,cr]]; this lane keeps row c
    const double F00 = cr * cr * d0 + sr * sr * d1, F01 = cr * sr * (d0 - d1), F11 = sr * sr * d0 + cr * cr * d1;
    const double Fc0 = c ? F01 : F00, Fc1 = c ? F11 : F01;
    const double dvp = gxor<G, 1>(dv);
    const double e0 = c ? dvp : dv, e1 = c ? dv : dvp;
    // E = Wv^T diag(e0,e1) Wv, Wv = [[cv,sv],[-sv,cv*s]]
    const double E00 = cv * cv * e0 + sv * sv * e1, E01 = cv * sv * e0 - sv * cv * foot_v * e1, E11 = sv * sv * e0 + cv * cv * e1;
    const double Ec0 = on * (c ? E01 : E00), Ec1 = on * (c ? E11 : E01);
    const double S0 = suffix_excl2<G>(Ec0, lane), S1 = suffix_excl2<G>(Ec1, lane);
    const double k2 = kap * kap;
    const double Pc0 = 2.0 * k2 * Ec0 + 4.0 * k2 * S0, Pc1 = 2.0 * k2 * Ec1 + 4.0 * k2 * S1;
    lds_P[grp][a][c][0] = Pc0; lds_P[grp][a][c][1] = Pc1;
    wave_sync();
    // P_max(a,b), row c, of every block b >= 1 as ONE 16-byte read each from stage max(a, b) -- for b <= a that is the pair
    // this lane has just written -- issued here, in front of the rest of the block arithmetic: no select on (b <= a), which
    // cost an exec-masked region with a read, a wait and a lane mask of its own per block.  Block 0 is always the lane's own
    // pair.  (lds_P holds LMAX stages, so lanes past the horizon and past the variable slots of the 8-variable bodies stay
    // in range: they read their own pair.)
    double q0[NMAX], q1[NMAX];
    q0[0] = Pc0; q1[0] = Pc1;
#pragma unroll
    for (int b = 1; b < NMAX; ++b) {
      const double2 pb = *reinterpret_cast<const double2*>(lds_P[grp][a > b ? a : b][c]);
      q0[b] = pb.x; q1[b] = pb.y;
    }
    // LDCBF block sum_t d_t eta eta^T of the stage: accumulated as (own own, own partner, partner partner); the two
    // lanes of a stage hold the same three sums with own / partner swapped
    double coo = c ? cys : cxs, cop = cxys, cpp = c ? cxs : cys;
#pragma unroll
    for (int t = 0; t < NOBS_R; ++t) {
      const double do_ = dc[t] * oo[t];
      coo = fma(do_, oo[t], coo); cop = fma(do_, oq[t], cop); cpp = fma(dc[t] * oq[t], oq[t], cpp);
    }
    coo += gxor<G, 1>(cpp); cop += gxor<G, 1>(cop);
    const double Cc0 = c ? cop : coo, Cc1 = c ? coo : cop;
    // F_{a+1}, row c (0 past the last stage: lanes without rows have d = 0, hence F = 0)
    const double Fn0 = gdown<G, 2>(Fc0, lane), Fn1 = gdown<G, 2>(Fc1, lane);
    const double Dg0 = (c ? 0.0 : 2.0) - k2 * Ec0 + Fc0 + Fn0 + Cc0;
    const double Dg1 = (c ? 2.0 : 0.0) - k2 * Ec1 + Fc1 + Fn1 + Cc1;
    // block b of the row: (-1)^(a+b) P_max(a,b) + [b==a] Dg - [b==a-1] F_a - [b==a+1] F_{a+1}; the three
    // indicator terms are FMAs against 0/1 masks (eqm), not selects.  Lanes/stages beyond N fall
    // out as rows of 2I because all their weights are zero.
#pragma unroll
    for (int b = 0; b < NMAX; ++b) {
      const double q0v = q0[b], q1v = q1[b];
      const double sg = sgn_a * ((b & 1) ? -1.0 : 1.0);
      double k0 = fma(eqm[b], Dg0, sg * q0v), k1 = fma(eqm[b], Dg1, sg * q1v);
      if (b + 1 < NMAX) { k0 = fma(-eqm[b + 1], Fc0, k0); k1 = fma(-eqm[b + 1], Fc1, k1); }
      if (b >= 1) { k0 = fma(-eqm[b - 1], Fn0, k0); k1 = fma(-eqm[b - 1], Fn1, k1); }
      Krow[2 * b] = k0;
      Krow[2 * b + 1] = k1;
    }
    wave_sync();
  };
  // Square-root-free right-looking factorisation K = Lt D^-1 Lt^T in full symmetric storage, one
  // row per lane, nothing rescaled: after step j lane j keeps row j of the Schur complement
  // (= column j of Lt, by symmetry) and lanes l > j keep Lt[l][j] in Krow[j]; ipiv = 1/pivot.
  // Per (j, c) that is one row_newbcast move and one FMA, with f = 0 on lanes <= j instead of
  // predication.  Returns false on a non-positive pivot.
  // G = 16: the pivot test is ONE running v_min_f64 per step (vmin, lipmpc_comm.hpp) and one comparison at the end, instead
  // of a comparison and a lane-mask OR per step (and an SGPR pair live across the whole factorisation).  It returns what
  // `ok = ok && (p_j > 0)` over all steps returns, for every input:
  //  * no pivot is NaN: min_j p_j > 0 exactly when every p_j > 0 (-0, +0 and -inf fail both forms; a denormal passes both;
  //    +inf passes the comparison in both -- as a pivot before the last its reciprocal is NaN, which is the next case);
  //  * some pivot is NaN: v_min_f64 returns its other operand, so the minimum alone would miss it.  But a NaN pivot p_j makes
  //    ip, then nf on every lane > j, then every K[cc], cc > j, on those lanes NaN (0 * NaN and inf * NaN are NaN too), so
  //    p_{j+1} -- K[j+1] of lane j + 1 -- and every later pivot is NaN: a NaN anywhere is a NaN in the LAST pivot, which is
  //    compared with 0 on its own.  (Pivots are results of FP arithmetic: never signalling.)
  double ipiv = 0.5;
  // broadcast inside the lane's own DPP row (16 lanes)
  auto bc16 = [](auto ic, double x) -> double {
    return __builtin_amdgcn_mov_dpp(x, 0x150 + decltype(ic)::value, 0xf, 0xf, false);
  };
  // G = 16: the triangular factors in the form the fused substitution steps want them (solve):
  //   Xl[j] = -Lt[l][j] / p_j on lanes l > j, 0 elsewhere;  Yu[j] = -Lt[j][l] / p_l ... = -ipiv_l S_l[j] on lanes l < j, 0 elsewhere
  double Xl[(FUSED || FUSED32_SOLVE) ? NV : 1], Yu[(FUSED || FUSED32_SOLVE) ? NV : 1];
  auto factor = [&]() -> bool {
    bool ok = true;
    const int ln = fresh(lane);
    dpp_fence();
    double pnext = 0.0;                                   // G = 16: pivot of the next step, broadcast at the end of the step
    if constexpr (FUSED) pnext = gbcast<G, 0>(Krow[0]);
    double pmin = pnext;                                  // G = 16: smallest pivot so far (NaN pivots skipped, see above)
    static_for<0, NV>([&](auto jc) {
      constexpr int j = decltype(jc)::value;
      if constexpr (FUSED) {
        // One DPP row per problem: pivot chain (broadcast, reciprocal, one Newton step, scaled column), then the NV - 1 - j
        // updates of the step as one asm statement.  (Issuing the updates BETWEEN the links of the next step's pivot chain --
        // "lookahead", tried in round 4 -- gains nothing: a dependent FP64 instruction costs 7 cycles against 4.6 for an
        // independent one, the chain is issue slots, not latency; profiles/r04_dev_tools/r04_iter_cost_lookahead_factorisation.txt.)
        const double pj = pnext;                          // gbcast<G, j>(Krow[j])
        if constexpr (j > 0) pmin = vmin(pmin, pj);
        if constexpr (j == NV - 1) ok = (pmin > 0.0) & (pj > 0.0);
        const double ip = fast_rcp(pj);
        const double nf = zero_unless(ln > j, Krow[j] * -ip);
        // ipiv ends as ip_l on lane l either way; (ln > j - 1) is the mask of the step before, (ln == j) one more compare.
        // (With NV < G the lanes past the variables keep 0.5: ln == j there.)
        ipiv = ((NV < G) ? (ln == j) : (ln > j - 1)) ? ip : ipiv;
        Xl[j] = nf;
        FactorStep<NV, j>::run(Krow, nf, pnext);
      } else {
        // Two DPP rows per problem.  Row j of the Schur complement equals its column j, and the column is lane-distributed
        // (lane cc holds S[cc][j] in Krow[j]): ONE cross-row exchange per step makes both 16-lane halves of the column
        // visible in every row, after which each update S[l][cc] -= (S[l][j] / p_j) S[cc][j] is one v_fmac_f64_dpp with the
        // broadcast of S[cc][j] as its DPP operand.  (LDL^T form: a Cholesky-form update g_l g_cc with g = S[.][j] / sqrt(p_j)
        // keeps the two triangles bit-identical but breaks down -- pivot <= 0 -- on 3 % of the N = 16 / 50-obstacle problems
        // where this form does not.)
        double cA, cB;                                    // S[0..15][j], S[16..31][j] by local lane position
        rowpair(Krow[j], cA, cB);
        const double pj = bc16(std::integral_constant<int, (j & 15)>{}, j < 16 ? cA : cB);
        ok = ok && (pj > 0.0);
        const double ip = fast_rcp(pj);
        ipiv = (ln == j) ? ip : ipiv;
        const double ng = zero_unless(ln > j, Krow[j] * -ip);
        if constexpr (FUSED32_SOLVE) Xl[j] = ng;
        FactorStep32<j>::run(Krow, cA, cB, ng);
      }
    });
    if constexpr (FUSED || FUSED32_SOLVE) {
      const double nip = -ipiv;
      static_for<1, NV>([&](auto jc) {
        constexpr int j = decltype(jc)::value;
        Yu[j] = zero_unless(ln < j, Krow[j] * nip);        // (ln: the one opaque copy of the lane index this call makes)
      });
    }
    return ok;
  };
  auto solve = [&](double b) -> double {
    const int ln = fresh(lane);
    if constexpr (FUSED) {
      // forward: b_l += Xl_l[j] b_j (lanes l > j); lane j's b is final after step j-1.  backward on x = w - ipiv acc:
      // x_l += Yu_l[j] x_j (lanes l < j), lane j final once the columns above it are done.  One instruction per step.
      dpp_fence();
      b = solve_forward_chain(b, Xl);
      return solve_backward_chain(b * ipiv, Yu);
    } else if constexpr (FUSED32_SOLVE) {
      // The same recurrences on two DPP rows, the substitution chain inside one row at a time (row_mask): columns 0..15
      // among the lanes of the low row, the high row catches up on those 16 columns after ONE cross-row exchange of the
      // finished values, columns 16..31 inside the high row; and the mirror image backwards.  Xl / Yu hold the
      // coefficients by group lane position (zero where a link does not apply), so a link is one v_fmac_f64_dpp.
      dpp_fence();
      b = solve32_fwd_lo(b, Xl);
      double lo_rep, hi_rep;
      rowpair(b, lo_rep, hi_rep);                         // lo_rep: the low row's b_0..b_15 by local lane position
      b = solve32_fwd_x(b, lo_rep, Xl);
      b = solve32_fwd_hi(b, Xl);
      double x = b * ipiv;
      x = solve32_bwd_hi(x, Yu);
      rowpair(x, lo_rep, hi_rep);                         // hi_rep: x_16..x_31
      x = solve32_bwd_x(x, hi_rep, Yu);
      return solve32_bwd_lo(x, Yu);
    } else {
      // Same recurrences, organised so that the substitution chain stays inside one DPP row at a time:
      // columns 0..15 are eliminated among the lanes of row 0, the lanes of row 1 catch up on those 16 columns
      // after ONE cross-row exchange of the finished w_0..w_15, then columns 16..31 run inside row 1
      // (and the mirror image backwards).
      const bool hi = (ln & 16) != 0;
      static_for<0, 16>([&](auto ic) {
        constexpr int j = decltype(ic)::value;
        const double wj = zero_unless(!hi && ln > j, bc16(ic, b * ipiv));
        b = fma(-Krow[j], wj, b);
      });
      {
        double wA, wB;
        rowpair(b * ipiv, wA, wB);                        // wA: w_0..w_15 by local lane position
        static_for<0, 16>([&](auto ic) {
          constexpr int j = decltype(ic)::value;
          b = fma(-Krow[j], zero_unless(hi, bc16(ic, wA)), b);
        });
      }
      static_for<0, 16>([&](auto ic) {
        constexpr int j = 16 + decltype(ic)::value;
        const double wj = zero_unless(hi && ln > j, bc16(ic, b * ipiv));
        b = fma(-Krow[j], wj, b);
      });
      const double w = b * ipiv;
      double acc = 0.0;
      static_rfor<16, 0>([&](auto ic) {
        constexpr int j = 16 + decltype(ic)::value;
        const double xj = zero_unless(hi && ln < j, bc16(ic, fma(-ipiv, acc, w)));
        acc = fma(Krow[j], xj, acc);
      });
      {
        double xA, xB;
        rowpair(fma(-ipiv, acc, w), xA, xB);              // xB: x_16..x_31 by local lane position
        static_for<0, 16>([&](auto ic) {
          constexpr int j = 16 + decltype(ic)::value;
          acc = fma(Krow[j], zero_unless(!hi, bc16(ic, xB)), acc);
        });
      }
      static_rfor<16, 0>([&](auto ic) {
        constexpr int j = decltype(ic)::value;
        const double xj = zero_unless(!hi && ln < j, bc16(ic, fma(-ipiv, acc, w)));
        acc = fma(Krow[j], xj, acc);
      });
      return fma(-ipiv, acc, w);
    }
  };
