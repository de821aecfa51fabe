// tests/hostsim -- TEST TOOLING ONLY: the verifier's U = s*G - c*pk and V = s*H - c*Gamma on the host build of one Edwards
// suite, staged as the kernels stage it: verify_decode_item's tables, k_verify.hip's load_cs_reduced, the two
// verify_straus_item halves, and the encoding of k_misc.hip's k_test_verify_uv_readout (one inversion, te_encode_affine).
// challenge_len replaces the suite string's for this call (the window the c ladders start from).  Returns 0, or 2 -- a point
// that does not decode / fails the subgroup test of check_mask, s >= r -- with zero bytes in u and v.
template <class S>
static uint32_t host_verify_uv(DevTables T, uint32_t challenge_len, uint32_t check_mask, const uint8_t* pk, const uint8_t* h,
                               const uint8_t* g, const uint8_t* c, const uint8_t* s, uint8_t* u, uint8_t* v) {
  T.sq.str.challenge_len = challenge_len;
  uint32_t w[5][8];
  memcpy(w[0], pk, 32); memcpy(w[1], h, 32); memcpy(w[2], g, 32); memcpy(w[3], c, 32); memcpy(w[4], s, 32);
  std::vector<uint32_t> tabs(VERIFY_TABS * WIN_TABLE_WORDS), uv(2 * UV_WORDS);
  bool valid = verify_decode_item<S>(T, w[0], w[1], w[2], tabs.data(), check_mask);
  uint32_t cr[8], c2[8], s2[8];
  fr_reduce256<S>(cr, w[3]);
  const bool canon = fr_is_canonical<S>(w[4]);
  for (int j = 0; j < 8; ++j) { c2[j] = canon ? cr[j] : 0; s2[j] = canon ? w[4][j] : 0; }
  verify_straus_item<S, 0>(uv.data(), T, tabs.data(), c2, s2);
  verify_straus_item<S, 1>(uv.data() + UV_WORDS, T, tabs.data(), c2, s2);
  valid = valid && canon;
  FeP zin[2] = {fe_load<1, 5>(uv.data() + 2 * NL), fe_load<1, 5>(uv.data() + UV_WORDS + 2 * NL)};
  FeN zi[2];
  fe_batch_inv(zi, zin);
  uint32_t e[2][8];
  te_encode_affine(e[0], fe_mul(fe_load<1, 5>(uv.data()), zi[0]), fe_mul(fe_load<1, 5>(uv.data() + NL), zi[0]), T.sq.str.flags);
  te_encode_affine(e[1], fe_mul(fe_load<1, 5>(uv.data() + UV_WORDS), zi[1]), fe_mul(fe_load<1, 5>(uv.data() + UV_WORDS + NL), zi[1]),
                   T.sq.str.flags);
  if (!valid) memset(e, 0, sizeof e);
  memcpy(u, e[0], 32); memcpy(v, e[1], 32);
  return valid ? 0 : 2;
}
