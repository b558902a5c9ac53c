// lipmpc_lidar_pieces.inc -- the optional stage between clustering and hulls of the sense kernels' body (lipmpc_lidar_body.inc): every
// cluster is cut into pieces of at most split_rays consecutive rays (the rule: include/lipmpc.h, lipmpc_lidar_c_eta_split_batch), and
// the pieces take the clusters' place.  In: rootr (cluster root of every reading), roots_ / n_clusters, the ray of every reading in
// cand_.  Out: rootr = piece number of every reading (NO_ROOT: none), roots_[k] = k, n_clusters = number of pieces -- what the hull
// stage reads, unchanged: its member lists are then the pieces'.  All integer arithmetic, all of it in registers: the members of a
// cluster are ballot masks (wave-uniform), a reading's predecessor in its cluster is a bit scan of them, and the only LDS traffic is
// the predecessor's ray.  No LDS of its own.
  {
    int ray[WORDS], piece[WORDS];
#pragma unroll
    for (int w = 0; w < WORDS; ++w) {
      const int i = w * 64 + lane;
      ray[w] = (i < n_pts) ? (int)cand_[i] : 0;
      piece[w] = NO_ROOT;
    }
    const int ncl = n_clusters < 64 ? n_clusters : 64;      // (clusters beyond the 64th have no root on record: the scan overflows)
    int n_pieces = 0;
    for (int k = 0; k < ncl; ++k) {
      const int r = roots_[k];
      // members of the cluster, ascending reading index = ascending ray; `before[w]`: its last member in the words below w
      unsigned long long mm[WORDS];
      int before[WORDS], last = -1;
#pragma unroll
      for (int w = 0; w < WORDS; ++w) {
        mm[w] = (w < NW) ? __ballot(rootr[w] == r) : 0ull;
        before[w] = last;
        if (mm[w]) last = w * 64 + 63 - __builtin_clzll(mm[w]);
      }
      if (last < 0) continue;                               // (cannot be: a root is a member of its cluster)
      // 1 + 2. the gap in front of every member, cyclically, and the anchor: the largest gap, the smallest ray on a tie --
      // one wave maximum of (gap, 511 - ray)
      int best = 0;
#pragma unroll
      for (int w = 0; w < WORDS; ++w) {
        if (w >= NW) continue;
        const bool m = (mm[w] >> lane) & 1ull;
        const unsigned long long below = mm[w] & ((1ull << lane) - 1ull);
        const int prev = below ? w * 64 + 63 - __builtin_clzll(below) : (before[w] >= 0 ? before[w] : last);
        int g = ray[w] - (int)cand_[m ? prev : 0];
        if (g <= 0) g += R;                                 // the first member looks back across ray 0 (a single member: gap R)
        const int key = (g << 9) | (511 - ray[w]);
        best = (m && key > best) ? key : best;
      }
      best = max(best, lipmpc_dev::row_xor<1>(best)); best = max(best, lipmpc_dev::row_xor<2>(best));
      best = max(best, lipmpc_dev::row_xor<4>(best)); best = max(best, lipmpc_dev::row_xor<8>(best));
      best = max(best, wave_xor16(best)); best = max(best, wave_xor32(best));
      best = __builtin_amdgcn_readfirstlane(best);
      // 3 - 6. offsets from the anchor; the extent is one past the offset of the member in front of the anchor, R - gap
      const int anchor = 511 - (best & 511);
      const int extent = R - (best >> 9) + 1;
      const int np = (extent + split - 1) / split;
#pragma unroll
      for (int w = 0; w < WORDS; ++w) {
        if (w >= NW) continue;
        int o = ray[w] - anchor;
        if (o < 0) o += R;
        const int p = (np == 1) ? 0 : (int)((unsigned)(o * np) / (unsigned)extent);
        if ((mm[w] >> lane) & 1ull) piece[w] = n_pieces + p;
      }
      n_pieces += np;
    }
    if (pieces_out) {
#pragma unroll
      for (int w = 0; w < WORDS; ++w) {
        const int i = w * 64 + lane;
        if (i < n_pts) pieces_out[b * R + ray[w]] = piece[w] == NO_ROOT ? -1 : piece[w];      // -1 noise
      }
    }
#pragma unroll
    for (int w = 0; w < WORDS; ++w) rootr[w] = piece[w];
    n_clusters = (n_clusters > 64 && n_pieces < 65) ? 65 : n_pieces;
    __syncthreads();                                        // roots_ has been read
    roots_[lane] = lane;                                    // (the hull stage's barrier comes before its first read)
  }
