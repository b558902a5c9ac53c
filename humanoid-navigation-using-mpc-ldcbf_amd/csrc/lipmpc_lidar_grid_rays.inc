// lipmpc_lidar_grid_rays.inc -- section 1 of lidar_grid_scan_kernel's body (lipmpc_lidar_body.inc): the scan of an OCCUPANCY GRID, the
// alternative to lipmpc_lidar_rays.inc.  In: the robot (x0, y0), the map (gm), the kernel arguments.  Out: n_pts readings in pint_, their
// rays in cand_ -- exactly what the polygon section leaves.  The arithmetic is the contract of lipmpc_lidar_grid_c_eta_batch
// (include/lipmpc.h), restated in numpy by tests/grid_lidar_oracle.py: contraction off, every operation in the order written there.
  // ---- 1. ray casting on a grid (Amanatides-Woo) ---------------------------------------------------
  {
#pragma clang fp contract(off)
    const unsigned char* occ = gm.occ + b * gm.stride;
    const int W = gm.W, H = gm.H;
    const double ox = gm.ox, oy = gm.oy, cdx = gm.dx, cdy = gm.dy;
    // the robot's cell; a robot no cell index below 2^30 in magnitude can be given to (far away, NaN) sees nothing
    const double fi = floor((x0 - ox) / cdx), fj = floor((y0 - oy) / cdy);
    const bool placed = (fabs(fi) < 1073741824.0) & (fabs(fj) < 1073741824.0);
    const int ci = placed ? (int)fi : 0, cj = placed ? (int)fj : 0;
    // The window: the cells within nx / ny = floor(range / cell) + 2 of the robot's.  A reading lies strictly within the range, i.e.
    // in a cell at most floor(range / cell) + 1 from the robot's; the cells beyond the window are never asked for.
    const int ww = 2 * gm.nx + 1, wh = 2 * gm.ny + 1, ncell = ww * wh;
    const int wi0 = ci - gm.nx, wj0 = cj - gm.ny;
    const bool meets = placed && ncell <= GRID_WINDOW_CELLS && wi0 < W && wi0 + ww > 0 && wj0 < H && wj0 + wh > 0;
    // a robot IN a solid cell has no scan: flagged (overflow), no reading
    const bool solid = placed && ci >= 0 && ci < W && cj >= 0 && cj < H && occ[(long)ci * H + cj] != 0;
    if (solid || ncell > GRID_WINDOW_CELLS) in_ovf = 1;
    double th[WORDS];                                 // ray parameter of the hit of ray lane + 64 p ...
    int hb[WORDS];                                    // ... the boundary it entered the solid cell through: index, bit 31 = a y boundary ...
    unsigned hitm = 0u;                               // ... where bit p is set
#pragma unroll
    for (int p = 0; p < WORDS; ++p) { th[p] = 0.0; hb[p] = 0; }
    if (meets && !solid) {
      // The window as a bitmap, bit li * wh + lj = cell (wi0 + li, wj0 + lj), cells outside the grid free: 64 cells per trip, one
      // byte per lane (consecutive lanes = consecutive j = consecutive bytes), the ballot is the word.  It lives where the polygon
      // section stages its edges (pint_: 6 KB = 49152 cells); the march then reads LDS only.
      unsigned long long* const bm64 = reinterpret_cast<unsigned long long*>(pint_);
      const int nchunk = (ncell + 63) >> 6;
      const int q64 = 64 / wh, r64 = 64 % wh;
      int li = lane / wh, lj = lane % wh;             // window cell of bit 64 c + lane
      int bi0 = ww, bi1 = -1, bj0 = wh, bj1 = -1;     // bounding box of the solid cells of the window
      for (int c = 0; c < nchunk; c += GRID_STAGE) {      // GRID_STAGE loads in flight per lane, then their ballots
        unsigned char v[GRID_STAGE];
        int vi[GRID_STAGE], vj[GRID_STAGE];
#pragma unroll
        for (int u = 0; u < GRID_STAGE; ++u) {
          const int gi = wi0 + li, gj = wj0 + lj;
          const bool in = (li < ww) & (gi >= 0) & (gi < W) & (gj >= 0) & (gj < H);
          v[u] = in ? occ[(long)gi * H + gj] : (unsigned char)0;
          vi[u] = li; vj[u] = lj;
          li += q64; lj += r64;
          if (lj >= wh) { lj -= wh; ++li; }
        }
#pragma unroll
        for (int u = 0; u < GRID_STAGE; ++u) {
          const unsigned long long ball = __ballot(v[u] != 0);
          if (lane == u && c + u < nchunk) bm64[c + u] = ball;
          if (v[u] != 0) { bi0 = min(bi0, vi[u]); bi1 = max(bi1, vi[u]); bj0 = min(bj0, vj[u]); bj1 = max(bj1, vj[u]); }
        }
      }
#pragma unroll
      for (int m = 1; m < 64; m <<= 1) {
        bi0 = min(bi0, __shfl_xor(bi0, m, 64)); bi1 = max(bi1, __shfl_xor(bi1, m, 64));
        bj0 = min(bj0, __shfl_xor(bj0, m, 64)); bj1 = max(bj1, __shfl_xor(bj1, m, 64));
      }
      __syncthreads();
      LIDAR_PHASE_END(6);
      const unsigned* const bm32 = reinterpret_cast<const unsigned*>(pint_);
      // The march, GRID_RAYS rays of a lane at a time (independent chains).  Per ray: t_x, t_y = the parameters at which it crosses
      // the next cell boundary in x / in y, each recomputed from the boundary's INDEX (no accumulated step); the smaller one is taken
      // (x on a tie), the ray is then in the next cell of that axis at parameter t; it stops beyond t = 1 (the end point), in the
      // first solid cell, or once it has passed the bounding box of the window's solid cells on the side it travels to (rays only
      // move away from the robot's cell: nothing solid lies ahead, which is the contract's window rule applied early).  A window
      // without a solid cell is not marched at all.
      for (int p0 = 0; p0 < WORDS; p0 += GRID_RAYS) {
        if (p0 * 64 >= R || bi1 < 0) break;
        double ivx[GRID_RAYS], ivy[GRID_RAYS], tx[GRID_RAYS], ty[GRID_RAYS];
        double ax[GRID_RAYS], ay[GRID_RAYS];             // index of the next x / y boundary ahead, as the double the crossing is formed from
        int ri[GRID_RAYS], rj[GRID_RAYS], rk[GRID_RAYS]; // window cell and its bit
        unsigned live = 0u, posx = 0u, posy = 0u;
#pragma unroll
        for (int g = 0; g < GRID_RAYS; ++g) {
          const int i = (p0 + g) * 64 + lane;
          const bool on = p0 + g < WORDS && i < R;
          const int i2 = on ? 2 * i : 0;
          const double ex = x0 + lidar_range * ray_table[i2], ey = y0 + lidar_range * ray_table[i2 + 1];
          const double rdx = on ? ex - x0 : 0.0, rdy = on ? ey - y0 : 0.0;
          ivx[g] = 1.0 / rdx; ivy[g] = 1.0 / rdy;
          if (rdx > 0.0) posx |= 1u << g;
          if (rdy > 0.0) posy |= 1u << g;
          ax[g] = (double)(ci + (rdx > 0.0 ? 1 : 0)); ay[g] = (double)(cj + (rdy > 0.0 ? 1 : 0));
          tx[g] = rdx != 0.0 ? ((ox + ax[g] * cdx) - x0) * ivx[g] : INFINITY;
          ty[g] = rdy != 0.0 ? ((oy + ay[g] * cdy) - y0) * ivy[g] : INFINITY;
          ri[g] = gm.nx; rj[g] = gm.ny; rk[g] = gm.nx * wh + gm.ny;
          if (on) live |= 1u << g;
        }
        while (__any(live != 0u)) {
#pragma unroll
          for (int g = 0; g < GRID_RAYS; ++g) {
            const bool mine = (live >> g) & 1u;
            if (!__any(mine)) continue;                  // every lane's ray g has ended
            if (!mine) continue;
            const bool xs = tx[g] <= ty[g];
            const double t = xs ? tx[g] : ty[g];
            const bool upx = (posx >> g) & 1u, upy = (posy >> g) & 1u;
            if (xs) {
              ri[g] += upx ? 1 : -1; rk[g] += upx ? wh : -wh; ax[g] += upx ? 1.0 : -1.0;
              tx[g] = ((ox + ax[g] * cdx) - x0) * ivx[g];
            } else {
              rj[g] += upy ? 1 : -1; rk[g] += upy ? 1 : -1; ay[g] += upy ? 1.0 : -1.0;
              ty[g] = ((oy + ay[g] * cdy) - y0) * ivy[g];
            }
            const bool ahead = (upx ? ri[g] <= bi1 : ri[g] >= bi0) & (upy ? rj[g] <= bj1 : rj[g] >= bj0);
            bool go = (t <= 1.0) & ahead;                // (a NaN parameter stops the ray; `ahead` keeps it in the window)
            if (go && ((bm32[rk[g] >> 5] >> (rk[g] & 31)) & 1u)) {
              // the boundary just crossed, relative to the window: the cell's near face (|index| < 2^16, the window is small)
              th[p0 + g] = t; hitm |= 1u << (p0 + g); go = false;
              hb[p0 + g] = xs ? ri[g] + (upx ? 0 : 1) : (int)(0x80000000u | (unsigned)(rj[g] + (upy ? 0 : 1)));
            }
            if (!go) live &= ~(1u << g);
          }
        }
      }
    }
    __syncthreads();                                  // the bitmap is dead: the readings go where it was
    // readings (hit + noise) compacted in ray order, as the polygon section leaves them
#pragma unroll
    for (int p = 0; p < WORDS; ++p) {
      const int i = p * 64 + lane;
      const bool on = i < R;
      const int i2 = on ? 2 * i : 0;
      const double ex = x0 + lidar_range * ray_table[i2], ey = y0 + lidar_range * ray_table[i2 + 1];
      const double rdx = ex - x0, rdy = ey - y0;
      // the coordinate of the axis that was crossed is the boundary's own (readings on one face of a wall are exactly in line,
      // as the polygon scan's are on an axis-parallel edge); the other one is that of x0 + t d
      const bool ycross = hb[p] < 0;
      const int ab = (ycross ? wj0 : wi0) + (hb[p] & 0x7fffffff);
      const double bc = (ycross ? oy : ox) + (double)ab * (ycross ? cdy : cdx);
      double qx = ycross ? x0 + th[p] * rdx : bc, qy = ycross ? bc : y0 + th[p] * rdy;
      const double dd = sqrt((qx - x0) * (qx - x0) + (qy - y0) * (qy - y0));
      const bool have = on & (((hitm >> p) & 1u) != 0u) & (dd < lidar_range);      // strictly inside the range, the polygon scan's rule
      if (!have) { qx = 0.0; qy = 0.0; }
      if (have && noise) { qx = qx + noise[(b * R + i) * 2]; qy = qy + noise[(b * R + i) * 2 + 1]; }
      if (hits_out && on) { hits_out[(b * R + i) * 2] = have ? qx : NAN; hits_out[(b * R + i) * 2 + 1] = have ? qy : NAN; }
      const unsigned long long ball = __ballot(have);
      if (have) {
        const int k = n_pts + __popcll(ball & ((1ull << lane) - 1ull));
        pint_[2 * k] = qx; pint_[2 * k + 1] = qy; cand_[k] = (unsigned short)i;
      }
      n_pts += __popcll(ball);
    }
    __syncthreads();
  }
