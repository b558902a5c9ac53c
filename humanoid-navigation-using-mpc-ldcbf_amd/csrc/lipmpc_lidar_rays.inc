// lipmpc_lidar_rays.inc -- section 1 of lidar_sense_kernel's body (lipmpc_lidar.hip): candidate obstacles, staged edges, the ray
// loops, the readings compacted in ray order.  In: the robot (x0, y0, exy, env), the kernel arguments.  Out: n_pts readings in pint_, their rays in cand_.
  // ---- 1. ray casting (compute_lidar_readings) ---------------------------------------------------
  // candidate obstacles: those whose bounding circle comes within the range (conservative: an obstacle that is
  // skipped cannot hold a point closer than lidar_range), compacted once per robot in list order
  for (int j0 = 0; j0 < n_env; j0 += 64) {
    const int j = j0 + lane;
    bool keep = false;
    double mx = 0.0, my = 0.0, rad = 0.0;
    if (j < n_env) {
      int nv = env[j];
      if (nv > v_env) { nv = v_env; in_ovf = 1; }
      const double* ring = exy + (long)j * v_env * 2;
      double rad2 = 0.0;
      if (v_env <= VFAST) {          // (wave-uniform) the whole ring in one round of loads: a loop of dependent loads is a loop of misses
        double vx[VFAST], vy[VFAST];
#pragma unroll
        for (int e = 0; e < VFAST; ++e) { const int ee = e < nv ? e : 0; vx[e] = nv > 0 ? ring[2 * ee] : 0.0; vy[e] = nv > 0 ? ring[2 * ee + 1] : 0.0; }
#pragma unroll
        for (int e = 0; e < VFAST; ++e) if (e < nv) { mx += vx[e]; my += vy[e]; }
        if (nv > 0) { mx /= nv; my /= nv; }
#pragma unroll
        for (int e = 0; e < VFAST; ++e) if (e < nv) rad2 = fmax(rad2, (vx[e] - mx) * (vx[e] - mx) + (vy[e] - my) * (vy[e] - my));
      } else {
        for (int e = 0; e < nv; ++e) { mx += ring[2 * e]; my += ring[2 * e + 1]; }
        if (nv > 0) { mx /= nv; my /= nv; }
        for (int e = 0; e < nv; ++e) rad2 = fmax(rad2, (ring[2 * e] - mx) * (ring[2 * e] - mx) + (ring[2 * e + 1] - my) * (ring[2 * e + 1] - my));
      }
      if (nv > 0) {
        rad = sqrt(rad2) * (1.0 + 1e-12);                  // (any circle around the ring does: the margins below cover the rounding)
        const double reach = (lidar_range + rad) * (1.0 + 1e-9) + 1e-9;
        keep = (mx - x0) * (mx - x0) + (my - y0) * (my - y0) <= reach * reach;
      }
    }
    const unsigned long long ball = __ballot(keep);
    if (keep) {
      const int k = n_cand + __popcll(ball & ((1ull << lane) - 1ull));
      if (k < RMAX) cand_[k] = (unsigned short)j;
      if (k < NCC) { candc_[k][0] = mx; candc_[k][1] = my; candc_[k][2] = rad; }
    }
    n_cand += __popcll(ball);
  }
  // cand_ holds RMAX obstacles: the (RMAX+1)-th obstacle in range is dropped and the scan flagged (overflow), never
  // read past the list
  if (n_cand > RMAX) { n_cand = RMAX; in_ovf = 1; }
  in_ovf = __any(in_ovf) ? 1 : 0;
  __syncthreads();
  LIDAR_PHASE_END(6);
  // this lane's rays (i = lane + 64 p): direction b1 - a1, nearest hit so far.  A ray beyond the resolution has a zero
  // direction: every denominator is 0, it never hits.
  double rdx[WORDS], rdy[WORDS], bd[WORDS], hx[WORDS], hy[WORDS];
  const double inv_len2 = 1.0 / (lidar_range * lidar_range);     // 1 / |ray|^2 for the sector test (an estimate with a margin)
#pragma unroll
  for (int p = 0; p < WORDS; ++p) {
#pragma clang fp contract(off)
    const int i = p * 64 + lane;
    const bool on = i < R;
    const double ex = x0 + lidar_range * (on ? ray_table[2 * i] : 0.0), ey = y0 + lidar_range * (on ? ray_table[2 * i + 1] : 0.0);
    rdx[p] = on ? ex - x0 : 0.0; rdy[p] = on ? ey - y0 : 0.0;
    bd[p] = lidar_range; hx[p] = 0.0; hy[p] = 0.0;
  }
  // The candidates' edges go through LDS in chunks of at most 64 obstacles / ECAP edges (one chunk on ordinary maps):
  // lane c stages candidate jc0 + c -- edge vector g = b2 - a2 and offset f = a1 - a2 of the ray origin, the two operands
  // compute_intersection (Utils/obstacles.py:107-123) forms from the edge -- then every pass of 64 rays walks the staged
  // edges in list order.  Hits are kept across chunks in registers.
  for (int jc0 = 0; jc0 < n_cand;) {
    const bool mine = jc0 + lane < n_cand;
    const int j = mine ? cand_[jc0 + lane] : 0;
    const int nv = mine ? min(env[j], v_env) : 0;
    int incl = nv;                                   // inclusive prefix sum of the edge counts over the lanes
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) { const int o = __shfl_up(incl, m, 64); if (lane >= m) incl += o; }
    const bool fits = mine && incl <= ECAP;          // a prefix of the lanes (incl is monotone)
    int nfit = __popcll(__ballot(fits));
    if (nfit == 0) { in_ovf = 1; nfit = 1; }         // one ring longer than ECAP edges: skipped and flagged
    if (fits) {
#pragma clang fp contract(off)
      const double* ring = exy + (long)j * v_env * 2;
      const int off = incl - nv;
      eoff_[lane] = off;
      auto put_edge = [&](int e, double ax, double ay, double bx, double by) {
#pragma clang fp contract(off)
        double* o = edge_ + 4 * (off + e);
        const double gx = bx - ax, gy = by - ay, fx = x0 - ax, fy = y0 - ay;
        o[0] = gx; o[1] = gy; o[2] = fx; o[3] = fy;
        nua_[off + e] = gx * fy - gy * fx;
      };
      if (v_env <= VFAST) {
        double vx[VFAST], vy[VFAST];
#pragma unroll
        for (int e = 0; e < VFAST; ++e) { const int ee = e < nv ? e : 0; vx[e] = nv > 0 ? ring[2 * ee] : 0.0; vy[e] = nv > 0 ? ring[2 * ee + 1] : 0.0; }
#pragma unroll
        for (int e = 0; e < VFAST; ++e)
          if (e < nv) { const bool last = e + 1 == nv; put_edge(e, vx[e], vy[e], last ? vx[0] : vx[(e + 1) % VFAST], last ? vy[0] : vy[(e + 1) % VFAST]); }
      } else {
        double ax = nv > 0 ? ring[0] : 0.0, ay = nv > 0 ? ring[1] : 0.0;
        const double fx0 = ax, fy0 = ay;
        for (int e = 0; e < nv; ++e) {
          const bool last = e + 1 == nv;
          const double bx = last ? fx0 : ring[2 * (e + 1)], by = last ? fy0 : ring[2 * (e + 1) + 1];
          put_edge(e, ax, ay, bx, by);
          ax = bx; ay = by;
        }
      }
      if (lane == nfit - 1) eoff_[nfit] = incl;
    } else if (lane == 0) { eoff_[0] = 0; eoff_[1] = 0; }      // (only when nothing fitted)
    __syncthreads();
    LIDAR_PHASE_END(7);
    for (int c = 0; c < nfit; ++c) {
      const int e0 = eoff_[c], e1 = eoff_[c + 1];
      const int jc = jc0 + c;
      double wx = 0.0, wy = 0.0, cr2 = INFINITY;
      if (jc < NCC) { wx = candc_[jc][0] - x0; wy = candc_[jc][1] - y0; const double cr = candc_[jc][2] + 1e-6; cr2 = cr * cr; }
#pragma unroll
      for (int p = 0; p < WORDS; ++p) {
        if (p * 64 >= R) continue;
        // sector test: the 64 rays of this pass span 64 degrees; an obstacle none of them comes near (distance from
        // its bounding circle's centre to the ray segment > radius, with a margin far above the rounding of this
        // estimate) is skipped by the whole wave — its edges could not have produced a hit for any of these rays
        {
          const double tt = fmin(1.0, fmax(0.0, (wx * rdx[p] + wy * rdy[p]) * inv_len2));
          const double ddx = wx - tt * rdx[p], ddy = wy - tt * rdy[p];
          if (!__any(ddx * ddx + ddy * ddy <= cr2)) continue;
        }
        // 0 <= ua <= 1 and 0 <= ub <= 1 for ua = nua / denom, ub = nub / denom decided WITHOUT dividing: a correctly
        // rounded quotient is >= 0 exactly when the signs agree (or the numerator is +-0) and <= 1 exactly when
        // |numerator| <= |denominator| (a quotient above 1 is at least 1 + 2^-53 (1 + tiny) and rounds to 1 + 2^-52;
        // the one unreachable exception: a negative quotient below 5e-324 in magnitude, which rounds to -0.0 >= 0).
        // Only a ray that really hits the edge pays for the division that places the hit.  Two edges per trip: their
        // tests are independent chains (the hits are then taken in edge order: ties keep the earlier edge).
        auto meets = [&](int e, double& nua, double& denom) {
#pragma clang fp contract(off)
          const double gx = edge_[4 * e], gy = edge_[4 * e + 1], fx = edge_[4 * e + 2], fy = edge_[4 * e + 3];
          denom = gy * rdx[p] - gx * rdy[p];
          nua = nua_[e];
          const double nub = rdx[p] * fy - rdy[p] * fx;
          const double ad = fabs(denom), sa = (denom > 0.0) ? nua : -nua, sb = (denom > 0.0) ? nub : -nub;
          return (denom != 0.0) & (sa >= 0.0) & (sa <= ad) & (sb >= 0.0) & (sb <= ad);
        };
        auto take = [&](double nua, double denom) {
#pragma clang fp contract(off)
          const double ua = nua / denom;
          const double qx = x0 + ua * rdx[p], qy = y0 + ua * rdy[p];
          const double dd = sqrt((qx - x0) * (qx - x0) + (qy - y0) * (qy - y0));
          if (dd < bd[p]) { bd[p] = dd; hx[p] = qx; hy[p] = qy; }      // strictly nearer: ties keep the earlier edge
        };
        int e = e0;
        for (; e + 1 < e1; e += 2) {
          double na, da, nb2, db;
          const bool ha = meets(e, na, da), hb = meets(e + 1, nb2, db);
          if (ha) take(na, da);
          if (hb) take(nb2, db);
        }
        if (e < e1) {
          double na, da;
          if (meets(e, na, da)) take(na, da);
        }
      }
    }
    __syncthreads();
    jc0 += nfit;
  }
  in_ovf = __any(in_ovf) ? 1 : 0;
  // Readings (hit + noise) go from the registers straight into the list compacted in ray order (typically 110-200 of 360 rays
  // return one): clustering and hulls then sweep n points instead of RMAX slots.  Order is preserved, so "smallest core index"
  // numbering, border-point assignment and every index tie-break are those of the uncompacted scan.  (The staged edges are
  // dead: the ray loop ends on a barrier.)
  n_pts = 0;
#pragma unroll
  for (int p = 0; p < WORDS; ++p) {
#pragma clang fp contract(off)
    const int i = p * 64 + lane;
    const bool have = bd[p] < lidar_range;           // bd starts at the range and only ever gets strictly smaller
    double qx = have ? hx[p] : 0.0, qy = have ? hy[p] : 0.0;
    if (have && noise) { qx = qx + noise[(b * R + i) * 2]; qy = qy + noise[(b * R + i) * 2 + 1]; }
    if (hits_out && i < R) { hits_out[(b * R + i) * 2] = have ? qx : NAN; hits_out[(b * R + i) * 2 + 1] = have ? qy : NAN; }
    const unsigned long long ball = __ballot(have);
    if (have) {
      const int k = n_pts + __popcll(ball & ((1ull << lane) - 1ull));
      pint_[2 * k] = qx; pint_[2 * k + 1] = qy; cand_[k] = (unsigned short)i;      // cand_ is free after the ray casting: ray of point k
    }
    n_pts += __popcll(ball);
  }
  __syncthreads();
