// tests/hostsim -- TEST TOOLING ONLY: per-proof Pedersen verification with the challenge supplied (vrfhip_test_pedersen_verify_c)
// on the host build of one Edwards suite, staged as k_pedersen.hip stages it: pedersen_verify_decode_item's tables and affine
// R, Ok, the override of k_ped_verify_set_c (challenge_supplied), the zeroing of out-of-range responses and the two
// pedersen_verify_straus_item halves, pedersen_verify_finish_item.  challenge_len replaces the suite string's for this call.
// Returns the status byte: 0, 1 (an equation fails), 2 (a point that does not decode / fails the subgroup test of check_mask,
// s or sb >= r, c >= 2^(8 challenge_len)).
template <class S>
static uint32_t host_pedersen_ladders_c(const DevTables& T, bool valid, const uint32_t* tabs, uint32_t* pts, const uint8_t* c,
                                        const uint8_t* s, const uint8_t* sb) {
  uint32_t cw[8], cr[8], sw[8], sbw[8], s2[8], sb2[8];
  memcpy(cw, c, 32); memcpy(sw, s, 32); memcpy(sbw, sb, 32);
  valid = challenge_supplied<S>(cr, cw, T.sq.str) && valid;
  const bool canon = fr_is_canonical<S>(sw) && fr_is_canonical<S>(sbw);
  for (int j = 0; j < 8; ++j) { s2[j] = canon ? sw[j] : 0; sb2[j] = canon ? sbw[j] : 0; }
  pedersen_verify_straus_item<S, 0>(pts, T, tabs, cr, s2, sb2);
  pedersen_verify_straus_item<S, 1>(pts + UV_WORDS, T, tabs, cr, s2, sb2);
  return pedersen_verify_finish_item<S>(pts, sw, sbw, valid);
}
template <class S>
static uint32_t host_pedersen_verify_c(DevTables T, uint32_t challenge_len, uint32_t check_mask, const uint8_t* h, const uint8_t* g,
                                       const uint8_t* pk_com, const uint8_t* r, const uint8_t* ok, const uint8_t* c,
                                       const uint8_t* s, const uint8_t* sb) {
  T.sq.str.challenge_len = challenge_len;
  uint32_t enc[5][8], hashed[8];
  memcpy(enc[0], h, 32); memcpy(enc[1], g, 32); memcpy(enc[2], pk_com, 32); memcpy(enc[3], r, 32); memcpy(enc[4], ok, 32);
  std::vector<uint32_t> tabs(VERIFY_TABS * WIN_TABLE_WORDS), pts(PROVE_PTS_WORDS);
  const bool valid = pedersen_verify_decode_item<S>(hashed, T, enc, nullptr, 0, tabs.data(), pts.data(), check_mask);
  return host_pedersen_ladders_c<S>(T, valid, tabs.data(), pts.data(), c, s, sb);
}
