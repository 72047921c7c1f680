// tpe_joint_pass.hpp -- the arithmetic the joint criterion's two scorers share
// (k_joint_score in tpe_joint.hip: a dense row window; k_joint_score_rows in
// tpe_joint_tree.hip: a device list of rows), as text: a thread's walk over one
// chunk of components, and a row's merge of its chunks.  Included inside the
// kernels' bodies, once per part (define TPE_JOINT_PASS_WALK or
// TPE_JOINT_PASS_MERGE first; no include guard).  Text, not a function: as an
// inlined function the same statements gave k_joint_score another scalar
// register assignment, and the dense scorer's code is to stay instruction for
// instruction what it was.
#if defined(TPE_JOINT_PASS_WALK)
#undef TPE_JOINT_PASS_WALK
// in:  labels, n_labels, tables, logw, sig, comp (the prepared set's parts), n,
//      C = n + 1, vals, ld, row (the pool row this thread reads), i_first (the
//      chunk's first component), tile (kJMaxD * kJPer JComp of LDS)
// out: m, s -- the running maximum and sum of the chunk's a_i.  Every thread
//      of the kJBS block walks it (it syncs on `tile`).
// With TPE_JOINT_PASS_CTX defined (k_joint_chain_rows in tpe_joint_chain.hip,
// which undefines it again) also in: n_ctx in (0, n_labels), and m_ctx = -inf,
// s_ctx = 0 declared by the kernel; out: m_ctx, s_ctx -- the same running pair
// over the a_i cut off after the first n_ctx labels.
  double m = kNegInf, s = 0.0;
  for (int64_t i0 = i_first; i0 < i_first + kJChunk && i0 < C; i0 += kJPer) {
    __syncthreads();  // (the previous pass has read the tile)
    for (int e = threadIdx.x; e < n_labels * kJPer; e += kJBS) {
      const int d = e / kJPer, k = e % kJPer;
      tile[e] = i0 + k < C ? comp[(int64_t)d * C + i0 + k] : JComp{0.0, 0.0};
    }
    __syncthreads();
    double a[kJPer];
#pragma unroll
    for (int k = 0; k < kJPer; ++k) a[k] = i0 + k < C ? logw[i0 + k] : kNegInf;
    const int k_prior = n - i0 < kJPer ? (int)(n - i0) : -1;  // the prior's place in this pass
    for (int d = 0; d < n_labels; ++d) {
#if defined(TPE_JOINT_PASS_CTX)
      // (k_joint_chain_rows alone defines it: the two scorers' text is unchanged)
      // at the label boundary a[] holds the a_i of the first n_ctx labels: it
      // joins a second running (m_ctx, s_ctx) by the pass's join below, word
      // for word, and the walk goes on to the full a_i in the same registers
      if (d == n_ctx) {
#pragma unroll
        for (int k = 0; k < kJPer; ++k)
          if (i0 + k >= C) a[k] = kNegInf;
        double pm = a[0];
#pragma unroll
        for (int k = 1; k < kJPer; ++k) pm = a[k] > pm ? a[k] : pm;
        if (pm > m_ctx) {
          s_ctx = s_ctx * exp(m_ctx - pm);
          m_ctx = pm;
        }
#pragma unroll 1
        for (int k = 0; k < kJPer; ++k) {
          const double head = a[0];
          s_ctx = s_ctx + (head == kNegInf ? 0.0 : exp(head - m_ctx));
#pragma unroll
          for (int j = 0; j + 1 < kJPer; ++j) a[j] = a[j + 1];
          a[kJPer - 1] = head;
        }
      }
#endif
      const tpe_joint_label lab = labels[d];
      const double x = vals[(int64_t)lab.col * ld + row];
      const JComp* __restrict__ t = tile + d * kJPer;
      if (lab.kind == TPE_JOINT_CONT) {
        const double tx = fit_coord(x, (lab.flags & TPE_JOINT_LOG) != 0);
        const double rt = sig[n_labels + d], rp = lab.prior_r;
#pragma unroll
        for (int k = 0; k < kJPer; ++k) {
          const double u = (tx - t[k].mu) * (k == k_prior ? rp : rt);
          a[k] = a[k] + fma(-u, u, t[k].cst);
        }
      } else if (lab.kind == TPE_JOINT_QUANT) {
        const bool is_log = (lab.flags & TPE_JOINT_LOG) != 0;
        const bool bounded = (lab.flags & TPE_JOINT_BOUNDED) != 0;
        const double lb = x - 0.5 * lab.q;
        double tu = fit_coord(x + 0.5 * lab.q, is_log), tl = fit_coord(lb, is_log);
        if (bounded) {
          tu = fmin(fmax(tu, lab.lo), lab.hi);
          tl = fmin(fmax(tl, lab.lo), lab.hi);
        } else if (is_log && lb <= 0.0) {
          tl = kNegInf;  // normal_cdf(-inf) is exactly 0
        }
        const double sigma = sig[d];
        // two erf and a log per component: a rolled loop (unrolled, the 32
        // erf bodies took the kernel to 188 VGPRs).  a[] stays in registers
        // because the loop rotates it by one place per step: every index is
        // static, and after kJPer steps the array is back in place.
#pragma unroll 1
        for (int k = 0; k < kJPer; ++k) {
          const double sg = k == k_prior ? lab.prior_sigma : sigma;
          const double head = a[0] + (log_mass(tu, tl, t[k].mu, sg) + t[k].cst);
#pragma unroll
          for (int j = 0; j + 1 < kJPer; ++j) a[j] = a[j + 1];
          a[kJPer - 1] = head;
        }
      } else {
        const int64_t c = llrint(x);
        const bool in = c >= 0 && c < lab.n_cat;  // (a validated pool: always)
        const double* __restrict__ tab = tables + lab.tab_off + (in ? c : 0);
        const double hit = in ? tab[0] : kNegInf, miss = in ? tab[lab.n_cat] : kNegInf;
        const double lp = in ? tab[2 * (int64_t)lab.n_cat] : kNegInf;
        const double xc = (double)c;
#pragma unroll
        for (int k = 0; k < kJPer; ++k)
          a[k] = a[k] + (k == k_prior ? lp : (t[k].mu == xc ? hit : miss));
      }
    }
    // a place past the last component holds no component: whatever the label
    // loop added to its -inf from the zero pad (a NaN where a factor was
    // inf * 0), it counts for nothing
#pragma unroll
    for (int k = 0; k < kJPer; ++k)
      if (i0 + k >= C) a[k] = kNegInf;
    // the pass joins the running (m, s), in component order
    double pm = a[0];
#pragma unroll
    for (int k = 1; k < kJPer; ++k) pm = a[k] > pm ? a[k] : pm;
    if (pm > m) {
      s = s * exp(m - pm);  // (m = -inf: s is 0 and stays 0)
      m = pm;
    }
#pragma unroll 1  // (rolled like the quantized loop: one exp body, a[] rotates)
    for (int k = 0; k < kJPer; ++k) {
      const double head = a[0];
      s = s + (head == kNegInf ? 0.0 : exp(head - m));
#pragma unroll
      for (int j = 0; j + 1 < kJPer; ++j) a[j] = a[j + 1];
      a[kJPer - 1] = head;
    }
  }
#elif defined(TPE_JOINT_PASS_MERGE)
#undef TPE_JOINT_PASS_MERGE
// in:  partial, n_chunks, n_rows (the partials' stride), r (the list position)
// out: v = log L from the row's partials in chunk order
  double m = kNegInf;
  for (int64_t c = 0; c < n_chunks; ++c) {
    const double pm = partial[c * n_rows + r].x;
    m = pm > m ? pm : m;
  }
  double s = 0.0;
  for (int64_t c = 0; c < n_chunks; ++c) {
    const double2 p = partial[c * n_rows + r];
    s = s + (p.x == kNegInf ? 0.0 : p.y * exp(p.x - m));
  }
  double v = m == kNegInf ? kNegInf : m + log(s);
#else
#error "tpe_joint_pass.hpp: define TPE_JOINT_PASS_WALK or TPE_JOINT_PASS_MERGE"
#endif
