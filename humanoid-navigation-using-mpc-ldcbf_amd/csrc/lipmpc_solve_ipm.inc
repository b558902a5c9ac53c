// lipmpc_solve_ipm.inc -- Mehrotra predictor-corrector on the normal equations (oracle: solve_qp_ipm), groups of a wave leaving the loop independently
// A SECTION OF THE BODY of step_solve (lipmpc_solve.hpp), included there: it shares that function's locals -- the lane
// constants, the row operators, the iterate -- and is no translation unit of its own.
  // ---- interior point ---------------------------------------------------------------------------
  const bool warm_on = warm != nullptr && warm->lds != nullptr;         // wave-uniform
  const bool warm_in = warm_on && warm->have;
  const bool last_stage = a >= N - 1;
  const int wsrc = last_stage ? lane : lane + 2;                          // stage a takes over stage a + 1; the last keeps its own
  double q = var_on ? p0c : 0.0;
  if (warm_in) {
    const double qo = warm->lds[lane], qn = warm->lds[wsrc], qb = warm->lds[lane >= 2 ? lane - 2 : lane];
    q = var_on ? (last_stage ? qo + (qo - qb) : qn) : 0.0;              // the last stage extrapolates one more step
  }
  double s[NR], z[NR], slk[NR];     // slack variable, multiplier, slack function value h - g.q
  double hl[NOBS_R > 0 ? NOBS_R : 1];
  double cx_ = 0.0, cy_ = 0.0;       // stage position / direction of the last rows_lin call, (x, y) order (streamed rows only)
  auto slack_values = [&](double x) {
    double r_lin, w_lin;
    rows_lin(x, r_lin, w_lin, hl, cx_, cy_);
    const double r = r_lin + r_c, w = w_lin + w_c;
    slk[R_RU] = hi_r - r; slk[R_RL] = r - lo_r;
    slk[R_VU] = hi_v - w; slk[R_VL] = w - lo_v;
    slk[R_M] = hi_m - w;
#pragma unroll
    for (int t = 0; t < NOBS_R; ++t) slk[R_CBF + t] = hl[t] - ob[t];
  };
  // g_i . dx for every local row from the linear maps
  auto rows_dir = [&](double dx, double (&dl)[NR]) {
    double r_lin, w_lin;
    rows_lin(dx, r_lin, w_lin, hl, cx_, cy_);
    dl[R_RU] = r_lin; dl[R_RL] = -r_lin; dl[R_VU] = w_lin; dl[R_VL] = -w_lin; dl[R_M] = cm * w_lin;
#pragma unroll
    for (int t = 0; t < NOBS_R; ++t) dl[R_CBF + t] = -hl[t];
  };
  auto GT_rows = [&](const double (&w)[NR], double axs, double ays) -> double {
    double wc[NOBS_R > 0 ? NOBS_R : 1];
#pragma unroll
    for (int t = 0; t < NOBS_R; ++t) wc[t] = w[R_CBF + t];
    return GT_apply(w[R_RU] - w[R_RL], fma(cm, w[R_M], w[R_VU] - w[R_VL]), wc, axs, ays);      // (cm: not the ballast row's slot)
  };
  auto K_rows = [&](const double (&d)[NR], double cxs, double cxys, double cys) {
    double dc[NOBS_R > 0 ? NOBS_R : 1];
#pragma unroll
    for (int t = 0; t < NOBS_R; ++t) dc[t] = d[R_CBF + t];
    form_K(d[R_RU] + d[R_RL], fma(cm, d[R_M], d[R_VU] + d[R_VL]), dc, cxs, cxys, cys);
  };

  slack_values(q);
  slk[R_M] = ball ? s_ball : slk[R_M];
  // An absent row (empty obstacle slot, manoeuvrability on the c = 1 lane, lane without a variable) is the constant
  // row 0 . q <= 1 with s = slk = 1, z = 0: its direction coefficients are zero, so r_p, ds, dz and its weights stay
  // exactly zero through the iteration with ONE masked quantity, 1/s (below), instead of a mask on every product.
#pragma unroll
  for (int i = 0; i < NR; ++i) {
    slk[i] = pres[i] ? slk[i] : 1.0;
    s[i] = pres[i] ? fmax(slk[i], IPM_S_FLOOR) : 1.0;
    z[i] = pres[i] ? IPM_Z0 : 1e-300;         // not 0: 1/z stays finite without a guard (a multiplier never reaches 0:
                                              // every step keeps at least 0.005 of it)
    if (warm_in && i < WARM_ROWS) z[i] = pres[i] ? fmin(fmax(warm->lds[(1 + i) * G + wsrc], WARM_Z_MIN), WARM_Z_MAX) : 1e-300;
  }
  if constexpr (STREAM) {
#pragma unroll STREAM_UNROLL
    for (int t = 0; t < NOBS_S; ++t) {
      double ex, ey, b;
      s_obs(t, ex, ey, b);
      const bool on = (pbits >> t) & 1u;
      lds_sz[grp][t][lane][0] = on ? fmax(ex * cx_ + ey * cy_ - b, IPM_S_FLOOR) : 1.0;
      lds_sz[grp][t][lane][1] = on ? IPM_Z0 : 0.0;
    }
  }
  // One streamed row as every pass sees it: (s, z) from LDS, the rest recomputed from (eta, b) and the
  // stage position (px, py) of the current iterate.
  struct SRow { double s, z, rp, is, d, ex, ey, pm; };
  auto s_row = [&](int t, double px, double py) -> SRow {
    SRow r;
    double b;
    s_obs(t, r.ex, r.ey, b);
    r.pm = s_pm(t);
    r.s = lds_sz[grp][t][lane][0]; r.z = lds_sz[grp][t][lane][1];
    r.rp = (r.s - (r.ex * px + r.ey * py - b)) * r.pm;
    r.is = fast_rcp(r.s);
    r.d = r.z * r.is;
    return r;
  };

  int status = LIPMPC_STATUS_MAX_ITER;
  int iters = 0;
  bool done = false;
  if (front_flag & 2) { status = LIPMPC_STATUS_DEGENERATE; done = true; }
  else if (front_flag & 1) { status = LIPMPC_STATUS_INFEASIBLE; done = true; }
  if (in.sensor_overflow) { status = LIPMPC_STATUS_SENSOR_OVERFLOW; done = true; }     // a truncated obstacle list is not planned against
  if (front_flag & 8) { status = LIPMPC_STATUS_MAX_ITER; done = true; }                // (never: the body was chosen by this very count)
  if (m_rows == 0.0 && !done) { status = LIPMPC_STATUS_SOLVED; done = true; q = var_on ? gc : 0.0; }

  // row-presence masks as 0/1 doubles: an absent row keeps s = 1, z = 0 and is neutralised by four
  // multiplies per iteration instead of predicated selects everywhere
  double pm[NR];
#pragma unroll
  for (int i = 0; i < NR; ++i) pm[i] = pres[i] ? 2.0 : 1.0;      // the Newton constant of 1/s (below)

  double rp[NR];                     // primal residual s - (h - g.q) of every row, carried through the iterations
#pragma unroll
  for (int i = 0; i < NR; ++i) rp[i] = s[i] - slk[i];
  // Groups of a wave leave the loop independently (real divergence: a finished group's lanes are
  // simply masked off; all exchanges inside are row-local DPP / group-local LDS).
  if (lane == 0) { lds_mu[grp][0] = INFINITY; lds_mu[grp][1] = 0.0; }
  PH(10)
  for (int it = 0; it <= P.max_iter; ++it) {
    if (__all(done)) break;
    if (!done) {
      // mu of the previous iteration (no-progress safeguard below), read HERE -- the factor of the iteration before is dead, the
      // register file at its emptiest -- and consumed after the mu reduction, so that its LDS round trip is off the chain.
      // (lds_read_here: an ordinary load is sunk into the lane-0 region that consumes it, right in front of its wait.)
      const double mu_prev = lds_read_here(&lds_mu[grp][0]);
      double w[NR], d[NR];
      double mu_l = 0.0, rpmax_l = 0.0, zmax_l = 0.0;
#pragma unroll
      for (int i = 0; i < NR; ++i) {                       // (vmax*: fmax without the canonicalisations, lipmpc_comm.hpp)
        mu_l = fma(s[i], z[i], mu_l);
        rpmax_l = i == 0 ? vmax0_abs(rp[i]) : vmax_abs(rpmax_l, rp[i]);
        zmax_l = i == 0 ? vmax0(z[i]) : vmax(zmax_l, z[i]);
      }
      mu_l = fma(ball_w * s[R_M], z[R_M], mu_l);           // the other n_d - 1 copies of the ballast row
      // streamed rows, pass A: residual statistics, K blocks and predictor weights in one sweep
      double qx = 0.0, qy = 0.0, cxs = 0.0, cxys = 0.0, cys = 0.0, axs = 0.0, ays = 0.0;
      if constexpr (STREAM) {
        const double qp = gxor<G, 1>(q);
        qx = c ? qp : q; qy = c ? q : qp;
#pragma unroll STREAM_UNROLL
        for (int t = 0; t < NOBS_S; ++t) {
          const SRow r = s_row(t, qx, qy);
          mu_l = fma(r.s, r.z, mu_l);
          rpmax_l = fmax(rpmax_l, fabs(r.rp));
          zmax_l = fmax(zmax_l, r.z);
          cxs = fma(r.d * r.ex, r.ex, cxs); cxys = fma(r.d * r.ex, r.ey, cxys); cys = fma(r.d * r.ey, r.ey, cys);
          const double wt = fma(r.d, r.rp - r.s, r.z);            // z + d (rp - s)
          axs = fma(r.ex, wt, axs); ays = fma(r.ey, wt, ays);
        }
      }
      const double musum = gsum<G>(mu_l);
      const double mu = musum * inv_m;
      // (every lane takes mu_prev here, behind mu, where it has long arrived: consumed only inside the lane-0 region below,
      // its wait would come back behind that region, as a wait for the region's own LDS write)
      double mu_prev_in = mu_prev;
      asm volatile("" : "+v"(mu_prev_in) : "v"(mu));
      {   // no-progress safeguard, a ramp in mu / mu_prev (oracle/lipmpc_oracle.py).  Both values live in LDS: one more
          // double kept in registers across the factorisation costs 5 % of the iteration in AGPR traffic.
        // (hardware reciprocal seed, 4.5e-8: the ramp is continuous, so that is as good as a division here)
        const double ramp = fmin(1.0, fmax(0.0, (mu * __builtin_amdgcn_rcp(mu_prev_in) - IPM_SLOW_RATIO) * (1.0 / (1.0 - IPM_SLOW_RATIO))));
        if (lane == 0) { lds_mu[grp][0] = mu; lds_mu[grp][1] = (it >= IPM_SLOW_FROM) ? IPM_SLOW_SIGMA * ramp : 0.0; }
      }
      // largest primal residual and the divergence test (z or |q| out of range, NaN included) in ONE group reduction: a
      // lane that sees divergence contributes +inf
      const double zq_l = fmax(zmax_l * (1.0 / IPM_Z_DIVERGE), fabs(q) * 1e-300);        // >= 1: diverged
      const double rpmax = gmax<G>(!(zq_l < 1.0) ? INFINITY : rpmax_l);
      const bool bad = !(rpmax < INFINITY);
      if (rpmax <= P.tol && mu <= P.tol) { status = LIPMPC_STATUS_SOLVED; done = true; iters = it; }
      else if (it == P.max_iter) { done = true; iters = it; }
      else if (bad) { status = LIPMPC_STATUS_INFEASIBLE; done = true; iters = it; }
      PH(0)
      if (!done) {
        // Reciprocals once per row and iteration; every later division becomes a multiply, and the
        // ratio tests run on -ds/s, -dz/z (largest ratio r => step 1/r) so they need no division.
        // 1/z only feeds a ratio test: the 4.5e-8-accurate hardware seed is enough there.
        double is_[NR];
#pragma unroll
        for (int i = 0; i < NR; ++i) {
          // 1/s by one Newton step on the hardware seed, y (c1 - s y) with c1 = 2; an absent row has s = 1 exactly
          // (seed exact) and c1 = 1, which makes its 1/s exactly 0: d, w, dz of that row vanish at no extra cost
          const double y0 = __builtin_amdgcn_rcp(s[i]);
          is_[i] = y0 * fma(-s[i], y0, pm[i]);
          d[i] = z[i] * is_[i];
        }
        K_rows(d, cxs, cxys, cys);
        PH(1)
        const bool fok = factor();
        PH(2)
        if (!fok) {
          // K loses numerical definiteness once max(z/s) ~ 1e15: near the solution that is
          // "converged to working precision" (the finish takes over), elsewhere infeasibility
          status = (rpmax <= IPM_STALL_TOL && mu <= IPM_STALL_TOL) ? LIPMPC_STATUS_SOLVED : LIPMPC_STATUS_INFEASIBLE;
          done = true; iters = it;
        }
        // right-hand sides  -r_d - G^T w = -2(q - g) - G^T (z + w): one transpose apply per solve.
        // predictor: rc = s z  ->  w = z (rp - s) / s
        const double m2qg = var_on ? -2.0 * (q - gc) : 0.0;
#pragma unroll
        for (int i = 0; i < NR; ++i) w[i] = fma(d[i], rp[i] - s[i], z[i]);
        const double dqa = solve(m2qg - GT_rows(w, axs, ays));
        // (the sigma floor of the safeguard, read behind the substitution chain: the predictor's row work hides its round trip)
        const double sigma_floor = lds_read_here(&lds_mu[grp][1]);
        PH(3)
        double dl[NR], c2[NR];                             // c2 = ds_aff dz_aff: all the corrector needs of the predictor
        rows_dir(dqa, dl);
        const double ax_ = cx_, ay_ = cy_;                  // predictor direction of this stage (streamed rows)
        double r_l = 1.0;                                  // largest of 1, -ds/s, -dz/z
        double s2_l = 0.0;                                 // sum ds dz: mu_aff = ((1 - a) sum(s z) + a^2 sum(ds dz)) / m,
                                                           // because s dz + z ds = -s z holds row by row for the predictor
#pragma unroll
        for (int i = 0; i < NR; ++i) {
          const double dsa = -rp[i] - dl[i];
          const double t = dsa * is_[i];                    // ds/s; and -dz/z = (s + ds)/s = 1 + t, no 1/z needed
          const double dza = -fma(d[i], dsa, z[i]);         // -(s z + z ds)/s
          r_l = fmax(r_l, fmax(-t, 1.0 + t));
          c2[i] = dsa * dza;
          s2_l += c2[i];
        }
        s2_l = fma(ball_w, c2[R_M], s2_l);
        if constexpr (STREAM) {                            // pass B
#pragma unroll STREAM_UNROLL
          for (int t = 0; t < NOBS_S; ++t) {
            const SRow r = s_row(t, qx, qy);
            const double dsa_t = (-r.rp + (r.ex * ax_ + r.ey * ay_)) * r.pm;      // g = -eta
            const double dza_t = -r.d * (r.s + dsa_t);
            r_l = fmax(r_l, fmax(-dsa_t * r.is, -dza_t * __builtin_amdgcn_rcp(fmax(r.z, 1e-300))));
            s2_l = fma(dsa_t, dza_t, s2_l);
          }
        }
        // reciprocals to 2e-15 (v_rcp_f64 + one Newton step) instead of IEEE divisions: five of them sat on the
        // iteration's serial chain at ~10 dependent instructions each
        const double a_aff = chain_rcp(gmax<G>(r_l));
        const double mu_aff = fma(a_aff * a_aff, gsum<G>(s2_l), (1.0 - a_aff) * musum) * inv_m;
        const double ratio = mu_aff * chain_rcp(mu);
        double sigma = ratio * ratio * ratio;
        sigma = vmax(sigma, sigma_floor);         // no-progress safeguard: floor computed at the top of the iteration
        const double sigma_mu = sigma * mu;
        PH(4)
        // corrector: rc = s z + ds_a dz_a - sigma mu
        double rc[NR];
#pragma unroll
        for (int i = 0; i < NR; ++i) {
          rc[i] = fma(s[i], z[i], c2[i]) - sigma_mu;
          w[i] = fma(fma(z[i], rp[i], -rc[i]), is_[i], z[i]);
        }
        axs = 0.0; ays = 0.0;
        if constexpr (STREAM) {                            // pass D
#pragma unroll STREAM_UNROLL
          for (int t = 0; t < NOBS_S; ++t) {
            const SRow r = s_row(t, qx, qy);
            const double dsa_t = (-r.rp + (r.ex * ax_ + r.ey * ay_)) * r.pm;
            const double dza_t = -r.d * (r.s + dsa_t);
            const double rc_t = (fma(r.s, r.z, dsa_t * dza_t) - sigma_mu) * r.pm;
            const double wt = fma(fma(r.z, r.rp, -rc_t), r.is, r.z);
            axs = fma(r.ex, wt, axs); ays = fma(r.ey, wt, ays);
          }
        }
        const double dq = solve(m2qg - GT_rows(w, axs, ays));
        PH(5)
        rows_dir(dq, dl);
        const double bx_ = cx_, by_ = cy_;                  // corrector direction of this stage
        r_l = IPM_STEP_FRAC;                               // alpha = min(1, 0.995 / max ratio)
        double ds[NR], dz[NR];
#pragma unroll
        for (int i = 0; i < NR; ++i) {
          ds[i] = -rp[i] - dl[i];
          dz[i] = -fma(z[i], ds[i], rc[i]) * is_[i];
          // 1/z only feeds this ratio test: the 4.5e-8-accurate hardware seed is enough
          r_l = fmax(r_l, fmax(-ds[i] * is_[i], -dz[i] * __builtin_amdgcn_rcp(z[i])));
        }
        // streamed rows: (ds, dz) of the combined direction, recomputed identically in passes E and F
        auto s_step = [&](const SRow& r, double& ds_t, double& dz_t) {
          const double dsa_t = (-r.rp + (r.ex * ax_ + r.ey * ay_)) * r.pm;
          const double dza_t = -r.d * (r.s + dsa_t);
          const double rc_t = (fma(r.s, r.z, dsa_t * dza_t) - sigma_mu) * r.pm;
          ds_t = (-r.rp + (r.ex * bx_ + r.ey * by_)) * r.pm;
          dz_t = -fma(r.z, ds_t, rc_t) * r.is;
        };
        if constexpr (STREAM) {                            // pass E
#pragma unroll STREAM_UNROLL
          for (int t = 0; t < NOBS_S; ++t) {
            const SRow r = s_row(t, qx, qy);
            double ds_t, dz_t;
            s_step(r, ds_t, dz_t);
            r_l = fmax(r_l, fmax(-ds_t * r.is, -dz_t * __builtin_amdgcn_rcp(fmax(r.z, 1e-300))));
          }
        }
        const double alpha = IPM_STEP_FRAC * chain_rcp(gmax<G>(r_l));
        if (!done) {
          if constexpr (STREAM) {                          // pass F (before q moves: rows are evaluated at the old iterate)
#pragma unroll STREAM_UNROLL
            for (int t = 0; t < NOBS_S; ++t) {
              const SRow r = s_row(t, qx, qy);
              double ds_t, dz_t;
              s_step(r, ds_t, dz_t);
              lds_sz[grp][t][lane][0] = fma(alpha, ds_t, r.s);
              lds_sz[grp][t][lane][1] = fma(alpha, dz_t, r.z);
            }
          }
          q = fma(alpha, dq, q);
          // the primal residual of a row shrinks by exactly 1 - alpha along a Newton step (ds + g.dq = -rp), so it is
          // carried by that recurrence instead of being re-formed from a slack value kept per row (one persistent double
          // per row less; the finish recomputes the slack functions from q)
          const double oma = 1.0 - alpha;
#pragma unroll
          for (int i = 0; i < NR; ++i) {
            s[i] = fma(alpha, ds[i], s[i]); z[i] = fma(alpha, dz[i], z[i]); rp[i] *= oma;
          }
        }
        PH(6)
      }
    }
  }
