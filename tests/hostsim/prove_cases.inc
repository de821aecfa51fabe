// tests/hostsim -- TEST TOOLING ONLY: the provers of an Edwards suite over a batch, staged as k_prove.hip stages them: stage 1 per
// item (k_prove_prepare) or K per lane from messages on the Elligator suite (k_prove_prepare_multi), stage 2 with the zeroed
// non-canonical scalar and the CT switch of k_prove_mul, stage 3 with K proofs per lane sharing one inversion (k_prove_finish:
// prove_encode_multi, prove_respond_item, the zeroed outputs of a refused item).  Included by the suites' host builds after their
// tables; tests/test_hostsim_prove_cases.py drives it.
// out: n x 288 B = gamma | c | s | pk (pk_com) | h | r | ok | sb | blinding; status: n bytes (0, or 2 = InvalidData)
template <class S>
static void host_prove_cases(const DevTables& T, int K, bool pedersen, bool ct, uint32_t n, const uint8_t* sk_arr, const uint8_t* msgs,
                             uint32_t msg_len, const uint8_t* inputs, const uint8_t* ad, uint32_t ad_len, uint32_t check_mask,
                             uint8_t* out, uint8_t* status) {
  constexpr int TW = ProveLayout<S>::TAB_WORDS, AUXW = 32;
  std::vector<uint32_t> tabs((size_t)n * TW), pts((size_t)n * PROVE_PTS_WORDS), aux((size_t)n * AUXW);
  std::vector<uint8_t> flags(n);
  bool multi = false;
  if constexpr (S::H2C_ELL2) {
    if (!inputs) {
      multi = true;
      BytesViewLite mv; mv.blob = msgs; mv.off = nullptr; mv.len = msg_len; mv.stride = msg_len;
      for (size_t first = 0; first < n; first += K)
        prove_prepare_multi<S>(K, T, first, n, sk_arr, mv, tabs.data(), pts.data(), aux.data(), AUXW, flags.data());
    }
  }
  for (size_t i = 0; i < n; ++i) {
    uint32_t sk[8], h_enc[8], k[8];
    memcpy(sk, sk_arr + 32 * i, 32);
    uint32_t* a = aux.data() + i * AUXW;
    if (!multi) {
      uint32_t hg[8];
      if (inputs) memcpy(hg, inputs + 32 * i, 32);
      const bool ok = prove_prepare_item<S>(h_enc, k, tabs.data() + i * TW, T, sk, inputs ? nullptr : msgs + (size_t)msg_len * i, msg_len,
                                            inputs ? hg : nullptr, 0, check_mask);
      for (int j = 0; j < 8; ++j) { a[j] = h_enc[j]; a[8 + j] = k[j]; }
      flags[i] = ok ? 1 : 0;
    }
    if (pedersen) {
      uint32_t b[8], kb[8];
      for (int j = 0; j < 8; ++j) h_enc[j] = a[j];
      pedersen_blinding<S>(b, sk, h_enc, ad, ad_len, T.sq.str);
      nonce_rfc8032<S>(kb, b, h_enc);
      for (int j = 0; j < 8; ++j) { a[16 + j] = b[j]; a[24 + j] = kb[j]; }
    }
  }
  for (size_t i = 0; i < n; ++i)
    for (int half = 0; half < 2; ++half) {
      uint32_t sc[8];
      if (half == 0) memcpy(sc, sk_arr + 32 * i, 32); else memcpy(sc, aux.data() + i * AUXW + 8, 32);
      if (!fr_is_canonical<S>(sc)) memset(sc, 0, 32);
      uint32_t* dst = pts.data() + i * PROVE_PTS_WORDS + half * 2 * UV_WORDS;
      const uint32_t* s2 = pedersen ? aux.data() + i * AUXW + 16 + half * 8 : nullptr;
      if (ct) prove_mul_item<S, true>(dst, T, tabs.data() + i * TW, sc, s2);
      else prove_mul_item<S, false>(dst, T, tabs.data() + i * TW, sc, s2);
    }
  for (size_t first = 0; first < n; first += K) {
    prove_encode_multi<S>(K, first, n, pts.data(), tabs.data(), TW, T.sq.str.flags);
    for (int jj = 0; jj < K; ++jj) {
      const size_t i = first + jj;
      if (i >= n) break;
      uint32_t sk[8], h_enc[8], k[8], c[8], s[8], o[4][8], sb[8] = {0}, b[8] = {0};
      memcpy(sk, sk_arr + 32 * i, 32);
      const uint32_t* a = aux.data() + i * AUXW;
      const uint32_t* enc = tabs.data() + i * TW + PROVE_ENC_OFF;
      memcpy(h_enc, a, 32); memcpy(k, a + 8, 32);
      memcpy(o[0], enc, 32); memcpy(o[1], enc + 8, 32); memcpy(o[2], enc + 16, 32); memcpy(o[3], enc + 24, 32);   // gamma, pk, ok, r
      prove_respond_item<S>(c, s, enc, h_enc, sk, k, ad, ad_len, T.sq.str);
      const bool ok = flags[i] != 0;
      if (pedersen) {
        uint32_t kb[8], cb[8];
        memcpy(b, a + 16, 32); memcpy(kb, a + 24, 32);
        fr_mul<S>(cb, c, b);
        fr_add<S>(sb, cb, kb);
      }
      if (!ok) {
        memset(o, 0, sizeof o); memset(c, 0, 32); memset(s, 0, 32); memset(sb, 0, 32); memset(b, 0, 32);
      }
      uint8_t* d = out + 288 * i;
      memcpy(d, o[0], 32); memcpy(d + 32, c, 32); memcpy(d + 64, s, 32); memcpy(d + 96, o[1], 32); memcpy(d + 128, h_enc, 32);
      memcpy(d + 160, o[3], 32); memcpy(d + 192, o[2], 32); memcpy(d + 224, sb, 32); memcpy(d + 256, b, 32);
      status[i] = ok ? 0 : 2;
    }
  }
}
