// tests/cpp_affine/affine_test.cpp -- the affine-point verifiers of the C++ mirror (include/vrfhip.hpp: ietf / pedersen
// verify, verify_batch, verify_batch_sharded over utils::XY) on the Bandersnatch golden vector, handed over by
// tests/test_cpp_affine.py as hex x || y points (decoded by the oracle), then on batches with tampered items.
//   affine_test <ad> <pk_xy> <h_xy> <gamma_xy> <c> <s>   <ped_ad> <pk_com_xy> <r_xy> <ok_xy> <ps> <psb>
// Exit code 0 = every check passed; prints the first failing check otherwise.
#include <cstdio>
#include <string>

#include "vrfhip.hpp"

using namespace ark_vrf_hip;
using S = BandersnatchSha512Ell2;

static Bytes unhex(const std::string& h) {
  Bytes b(h.size() / 2);
  for (size_t i = 0; i < b.size(); ++i) b[i] = (uint8_t)std::stoul(h.substr(2 * i, 2), nullptr, 16);
  return b;
}
template <class A>
static A arr(const std::string& h) {
  A a{};
  Bytes b = unhex(h);
  if (b.size() != a.size()) throw std::invalid_argument("bad length: " + h);
  std::copy(b.begin(), b.end(), a.begin());
  return a;
}
#define CHECK(cond)                                                        \
  do {                                                                     \
    if (!(cond)) { std::printf("FAILED: %s (line %d)\n", #cond, __LINE__); return 1; } \
  } while (0)

static const Result OK = std::nullopt;
static const Result VF = Error::VerificationFailure;
static const Result ID = Error::InvalidData;

int main(int argc, char** argv) {
  if (argc != 13) { std::printf("usage: see the header of affine_test.cpp\n"); return 2; }
  auto A = [&](int i) { return std::string(argv[i]); };
  Context<S> ctx(0), ctx2(0);
  const std::vector<const Context<S>*> both = {&ctx, &ctx2};

  // ---- IETF ----
  const Bytes ad = unhex(A(1));
  ietf::ItemXY<S> it{arr<utils::XY>(A(2)), arr<utils::XY>(A(3)), arr<utils::XY>(A(4)), {arr<Scalar>(A(5)), arr<Scalar>(A(6))}};
  CHECK(ietf::verify(ctx, it.pub, it.input, it.output, ad, it.proof) == OK);
  ietf::ItemXY<S> bad_s = it;
  bad_s.proof.s[0] ^= 1;
  CHECK(ietf::verify(ctx, bad_s.pub, bad_s.input, bad_s.output, ad, bad_s.proof) == VF);
  ietf::ItemXY<S> off = it;
  off.output[40] ^= 1;                                   // y of Gamma changed: off the curve
  std::vector<ietf::ItemXY<S>> ib = {it, bad_s, off, it, it};
  const std::vector<Result> iw = {OK, VF, ID, OK, OK};
  CHECK(ietf::verify_batch(ctx, ib, ad) == iw);
  CHECK(ietf::verify_batch_sharded(both, ib, ad) == iw);

  // ---- Pedersen ----
  const Bytes pad = unhex(A(7));
  pedersen::ItemXY<S> pt{it.input, it.output,
                         {arr<utils::XY>(A(8)), arr<utils::XY>(A(9)), arr<utils::XY>(A(10)), arr<Scalar>(A(11)), arr<Scalar>(A(12))}};
  CHECK(pedersen::verify(ctx, pt.input, pt.output, pad, pt.proof) == OK);
  pedersen::ItemXY<S> bad_sb = pt;
  bad_sb.proof.sb[1] ^= 4;
  CHECK(pedersen::verify(ctx, bad_sb.input, bad_sb.output, pad, bad_sb.proof) == VF);
  pedersen::ItemXY<S> big = pt;
  for (int j = 0; j < 32; ++j) big.proof.r[j] = 0xff;    // x of R >= q: no such point
  std::vector<pedersen::ItemXY<S>> pb = {pt, bad_sb, big, pt};
  const std::vector<Result> pw = {OK, VF, ID, OK};
  CHECK(pedersen::verify_batch(ctx, pb, pad) == pw);
  CHECK(pedersen::verify_batch_sharded(both, pb, pad) == pw);
  CHECK(pedersen::verify_batch_sharded(both, pb, pad, true) == pw);
  std::vector<pedersen::ItemXY<S>> good(3, pt);
  CHECK(pedersen::verify_batch_sharded(both, good, pad, true) == std::vector<Result>(3, OK));
  std::printf("affine_test ok\n");
  return 0;
}
