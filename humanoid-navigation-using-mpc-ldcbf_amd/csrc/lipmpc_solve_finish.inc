// lipmpc_solve_finish.inc -- end of the interior-point phase (ballast row, warm-start parking, canonical row indices, initial working set) and the certified primal active-set finish (oracle: finish_active_set)
// A SECTION OF THE BODY of step_solve (lipmpc_solve.hpp), included there: it shares that function's locals -- the lane
// constants, the row operators, the iterate -- and is no translation unit of its own.
  if (ball) { pres.set(R_M, false); s[R_M] = 1.0; z[R_M] = 0.0; }      // the ballast row ends with the interior-point phase
  if (warm_on) {                              // park this step's interior-point result for the next step
    wave_sync();                              // (every lane has read its neighbours' previous values by now)
    warm->lds[lane] = q;
#pragma unroll
    for (int i = 0; i < NR && i < WARM_ROWS; ++i) {
      if constexpr (RECORD) warm->lds[(1 + i) * G + lane] = pres[i] ? z[i] : 0.0;
      else warm->lds[(1 + i) * G + lane] = z[i];
    }
    wave_sync();
  }
  // canonical row index (include/lipmpc.h) of a local row slot / of streamed row t
  const CanonicalRows ci_of{a, c, N, P, perm};
  auto ci_s = [&](int t) -> int { return ci_of.ldcbf(t); };

  // diagnostics: identification margin min |log(z/(1e5 s))| and final mu of the interior-point phase;
  // initial working set z > 1e5 s
  // (the logarithms cost ~2 us per wave: only when the caller asked for diag)
  double marg_l = INFINITY;
  const bool want_diag = diag != nullptr;
  RowFlags act;
  unsigned abits = 0u;
#pragma unroll
  for (int i = 0; i < NR; ++i) {
    if (want_diag && pres[i]) marg_l = fmin(marg_l, fabs(log(z[i] / (FIN_IDENT * s[i]))));
    act.set(i, pres[i] && (z[i] > FIN_IDENT * s[i]));
  }
  if constexpr (STREAM) {
#pragma unroll STREAM_UNROLL
    for (int t = 0; t < NOBS_S; ++t) {
      if ((pbits >> t) & 1u) {
        const double st = lds_sz[grp][t][lane][0], zt = lds_sz[grp][t][lane][1];
        if (want_diag) marg_l = fmin(marg_l, fabs(log(zt / (FIN_IDENT * st))));
        if (zt > FIN_IDENT * st) abits |= 1u << t;
      }
    }
  }
  const unsigned fbits = abits;          // fallback working set of an uncertified finish
  const double margin = gmin<G>(marg_l);
  double diag_rounds = 0.0, diag_eres = 0.0, diag_cert = 0.0;

  // ---- certified active-set finish --------------------------------------------------------------
  // A PRIMAL active-set method from the interior-point iterate (oracle: finish_active_set): per round one factorisation of
  // K_A = 2I + rho G_A^T G_A, the minimiser x_A on the working set by the method of multipliers, a ratio test along
  // d = x_A - x over the rows outside A (a blocked step stops at the blocking row, which joins A), otherwise the rows
  // with a negative multiplier leave A, otherwise x_A is the optimum.  x stays feasible, the objective never increases, and a
  // blocking row is never dependent on A (g.d = 0 for every row in A's span), which is what the degenerate vertices of
  // the long-horizon / many-obstacle problems need.
  const bool ipm_ok = (status == LIPMPC_STATUS_SOLVED) && (m_rows > 0.0);
  if (!(P.flags & LIPMPC_FLAG_INTERIOR)) {
    bool fin_done = !ipm_ok;        // groups that never converged skip the finish
    bool certified = false;
    double rho = FIN_RHO;           // penalty of the equality solves (FIN_RHO_POLISH after a polish request, below)
    double xf = q;                  // the feasible point the rounds move
    double qf = q;                  // minimiser on the working set
    double y[NR];
#pragma unroll
    for (int i = 0; i < NR; ++i) y[i] = act[i] ? z[i] : 0.0;
    if constexpr (STREAM) {           // the z slot of a streamed row now holds its multiplier y
#pragma unroll STREAM_UNROLL
      for (int t = 0; t < NOBS_S; ++t)
        if (!((abits >> t) & 1u)) lds_sz[grp][t][lane][1] = 0.0;
    }
    // slack function of streamed row t at the stage position / its ratio-test entry: evaluated twice per round (value,
    // then index of the minimum), so both evaluations must round alike
    auto s_slack = [&](int t, double fx, double fy) -> double {
#pragma clang fp contract(off)
      double ex, ey, bb;
      s_obs(t, ex, ey, bb);
      return ex * fx + ey * fy - bb;
    };
    auto s_ratio = [&](int t, double fx, double fy, double ddx, double ddy) -> double {
#pragma clang fp contract(off)
      double ex, ey, bb;
      s_obs(t, ex, ey, bb);
      const double sl = ex * fx + ey * fy - bb, gd = -(ex * ddx + ey * ddy);       // g = -eta
      const bool cand = gd > FIN_GD_MIN;
      return cand ? fmax(sl + gd, 0.0) * fast_rcp(gd) : INFINITY;
    };
    for (int rnd = 0; rnd < P.fin_rounds; ++rnd) {
      if (__all(fin_done)) break;
      double d[NR];
#pragma unroll
      for (int i = 0; i < NR; ++i) d[i] = act[i] ? rho : 0.0;
      double cxs = 0.0, cxys = 0.0, cys = 0.0;
      if constexpr (STREAM) {
#pragma unroll STREAM_UNROLL
        for (int t = 0; t < NOBS_S; ++t) {
          if ((abits >> t) & 1u) {
            double ex, ey, bb;
            s_obs(t, ex, ey, bb);
            cxs = fma(rho * ex, ex, cxs); cxys = fma(rho * ex, ey, cxys); cys = fma(rho * ey, ey, cys);
          }
        }
      }
      PH(9)
      K_rows(d, cxs, cxys, cys);
      const bool fok = factor();
      PH(7)
      qf = xf;                                         // the equality solve starts at the current point
      double eres = INFINITY, rd_g = 0.0, r_g = 0.0;
      for (int in = 0; in <= FIN_INNER; ++in) {
        slack_values(qf);
        const double fx = cx_, fy = cy_;               // stage position of qf
        double wr[NR], rmax_l = 0.0;
#pragma unroll
        for (int i = 0; i < NR; ++i) {
          const double r = act[i] ? -slk[i] : 0.0;      // G_A q - h_A
          wr[i] = -d[i] * slk[i];                       // rho r (d = rho on active rows, 0 elsewhere)
          // (vmax*, vmin: fmax / fmin without the canonicalisation of every selected operand, lipmpc_comm.hpp)
          rmax_l = i == 0 ? vmax0_abs(r) : vmax_abs(rmax_l, r);
        }
        double ayx = 0.0, ayy = 0.0, awx = 0.0, awy = 0.0;
        if constexpr (STREAM) {
#pragma unroll STREAM_UNROLL
          for (int t = 0; t < NOBS_S; ++t) {
            if ((abits >> t) & 1u) {
              double ex, ey, bb;
              s_obs(t, ex, ey, bb);
              const double r = -(ex * fx + ey * fy - bb);
              const double yt = lds_sz[grp][t][lane][1];
              rmax_l = fmax(rmax_l, fabs(r));
              ayx = fma(ex, yt, ayx); ayy = fma(ey, yt, ayy);
              awx = fma(ex, rho * r, awx); awy = fma(ey, rho * r, awy);
            }
          }
        }
        const double gty = GT_rows(y, ayx, ayy);
        const double rd = var_on ? (2.0 * (qf - gc) + gty) : 0.0;
        const double eprev = eres;
        rd_g = gmax<G>(fabs(rd));
        r_g = gmax<G>(rmax_l);
        eres = vmax(rd_g, r_g);
        // converged, out of corrections, or stalled on its rounding floor below what the certificate needs (an
        // ill-conditioned working set sits at 1e-10 forever: four corrections of ~1.7 us each, per round, for nothing)
        const bool stop = (eres <= FIN_INNER_TOL) || (in == FIN_INNER) || (eres <= FIN_EPS && eres > FIN_STALL * eprev);
        if (__all(stop || fin_done)) break;
        const double dq = solve(-rd - GT_rows(wr, awx, awy));
        double dl[NR];
        rows_dir(dq, dl);
        if (!stop && !fin_done) {
          qf += dq;
#pragma unroll
          for (int i = 0; i < NR; ++i) y[i] = fma(d[i], dl[i] - slk[i], y[i]);     // rho on active rows only
          if constexpr (STREAM) {
            const double ddx = cx_, ddy = cy_;
#pragma unroll STREAM_UNROLL
            for (int t = 0; t < NOBS_S; ++t) {
              if ((abits >> t) & 1u) {
                double ex, ey, bb;
                s_obs(t, ex, ey, bb);
                const double slk_t = ex * fx + ey * fy - bb, dl_t = -(ex * ddx + ey * ddy);
                lds_sz[grp][t][lane][1] += rho * (dl_t - slk_t);
              }
            }
          }
        }
      }
      PH(8)
      // (slk holds the slack functions of the final qf: every pass of the loop above evaluates them before it decides to stop)
      // ratio test along d = qf - xf: slack at x = slack at qf + g.d; entry of a row outside A the direction runs into:
      // max(slack at x, 0) / g.d; the smallest entry below 1 blocks the step
      const double fx = cx_, fy = cy_;                  // stage position of qf (streamed rows)
      const double dd = qf - xf;
      double gd[NR], rr[NR];
      rows_dir(dd, gd);
      const double ddx = cx_, ddy = cy_;                // stage direction
      double rbest = INFINITY;
#pragma unroll
      for (int i = 0; i < NR; ++i) {
        const bool cand = pres[i] & !act[i] & (gd[i] > FIN_GD_MIN);
        // (reciprocal to 2e-15 instead of the IEEE division of the oracles: 26 instead of 74 cycles per row on the round's
        // serial path; the last bit of a ratio only matters on an exact tie between two blocking rows)
        rr[i] = cand ? fmax(slk[i] + gd[i], 0.0) * fast_rcp(gd[i]) : INFINITY;
        rbest = fmin(rbest, rr[i]);
      }
      // multipliers on A and slack functions outside A at qf: the VALUES first (group extrema).  Most rounds end here,
      // certified, and never look at a row index; only a group that has to exchange a row finds which one: the lowest
      // canonical index among the rows attaining the extremum (numpy's argmin order), one integer group minimum each.
      double ymin = INFINITY, ymax = 0.0, smin = INFINITY;
#pragma unroll
      for (int i = 0; i < NR; ++i) {
        const bool ta = act[i], ti = pres[i] & !ta;
        const double ylo = ta ? y[i] : INFINITY, yhi = ta ? y[i] : 0.0, slo = ti ? slk[i] : INFINITY;
        ymin = i == 0 ? fmin(ymin, ylo) : vmin(ymin, ylo);
        ymax = i == 0 ? vmax0(yhi) : vmax(ymax, yhi);
        smin = i == 0 ? fmin(smin, slo) : vmin(smin, slo);
      }
      if constexpr (STREAM) {
#pragma unroll STREAM_UNROLL
        for (int t = 0; t < NOBS_S; ++t) {
          if ((pbits >> t) & 1u) {
            if ((abits >> t) & 1u) { const double yt = lds_sz[grp][t][lane][1]; ymin = fmin(ymin, yt); ymax = fmax(ymax, yt); }
            else { smin = fmin(smin, s_slack(t, fx, fy)); rbest = fmin(rbest, s_ratio(t, fx, fy, ddx, ddy)); }
          }
        }
      }
      rbest = gmin<G>(rbest);
      ymin = gmin<G>(ymin);
      int bi = 0x7fffffff;
      const bool blocked = !fin_done & (rbest < 1.0);
      const bool dropping = !fin_done & !blocked & (ymin < -FIN_EPS);
      if (__any(blocked)) {                         // which row blocks: lowest canonical index among the rows at the minimum
#pragma unroll
        for (int i = 0; i < NR; ++i) {
          const int ci = ci_of(i);
          bi = ((rr[i] == rbest) & (ci < bi)) ? ci : bi;          // (rr is finite on candidates only)
        }
        if constexpr (STREAM) {
#pragma unroll STREAM_UNROLL
          for (int t = 0; t < NOBS_S; ++t) {
            if (((pbits >> t) & 1u) && !((abits >> t) & 1u)) {
              const int ci = ci_s(t);
              if (s_ratio(t, fx, fy, ddx, ddy) == rbest && ci < bi) bi = ci;
            }
          }
        }
        bi = gmin_int<G>(bi);
      }
      if (__any(blocked | dropping)) {
        // register rows by selects (the groups of a wave take different arms): the blocking row joins; every row with a
        // negative multiplier leaves
#pragma unroll
        for (int i = 0; i < NR; ++i) {
          const bool hd = dropping & act[i] & (y[i] < -FIN_EPS), ha = blocked & pres[i] & !act[i] & (ci_of(i) == bi);
          y[i] = hd ? 0.0 : y[i];
          act.m = (act.m & ~((unsigned)hd << i)) | ((unsigned)ha << i);
        }
        if constexpr (STREAM) {
#pragma unroll STREAM_UNROLL
          for (int t = 0; t < NOBS_S; ++t) {
            const bool on_t = (pbits >> t) & 1u, act_t = (abits >> t) & 1u;
            if (dropping && act_t && lds_sz[grp][t][lane][1] < -FIN_EPS) { abits &= ~(1u << t); lds_sz[grp][t][lane][1] = 0.0; }
            if (blocked && on_t && !act_t && ci_s(t) == bi) abits |= 1u << t;
          }
        }
      }
      if (!fin_done) {
        if (blocked) {
          xf = fma(rbest, dd, xf);
        } else {
          xf = qf;
          // polish: an equality solve left above FIN_POLISH_TOL (two active rows a few 1e-6 from parallel: the multiplier
          // iteration contracts that direction by 2 / (2 + rho sigma^2) per correction only) gets one more round on the
          // same set at the stiffer penalty before it may certify
          const bool polish = !dropping & (eres > FIN_POLISH_TOL) & (rho == FIN_RHO) & (rnd + 1 < P.fin_rounds);
          rho = polish ? FIN_RHO_POLISH : rho;
          if (!dropping && !polish) {
            ymax = gmax<G>(ymax);
            smin = gmin<G>(smin);
            const double qabs = gmax<G>(fabs(qf));
            fin_done = true;
            certified = fok && (r_g <= FIN_EPS) && (rd_g <= FIN_EPS + FIN_DUAL_REL * ymax) && (smin >= -FIN_EPS) && (qabs < 1e300);
            diag_cert = vmin(ymin, smin);      // how decisively the certificate holds (weakly active rows -> ~0)
          }
        }
        diag_rounds = rnd + 1;
        diag_eres = eres;
      }
    }
    if (ipm_ok) {
      if (certified) {
        q = xf;
      } else {
        status = LIPMPC_STATUS_UNCERTIFIED;
#pragma unroll
        for (int i = 0; i < NR; ++i) act.set(i, pres[i] && (z[i] > FIN_IDENT * s[i]));
        abits = fbits;
      }
    }
  }

  PH(9)
