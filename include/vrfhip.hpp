// vrfhip.hpp -- C++ host-side mirror of the `ark-ec-vrfs` / `ark-vrf` API over the C ABI (vrfhip.h).
//
// The reference is a Rust crate whose whole surface is the re-export list at /root/reference src/lib.rs:13-17
// (`Suite`, `Secret`, `Public`, `Input`, `Output`, `ietf`, `pedersen`, `Error`, `codec`).  There is no Rust
// toolchain in this image, so the host side above the C ABI is written in C++ with the reference's names,
// argument order and error behaviour; INTEGRATION.md shows the equivalent Rust binding.  Header-only; every
// call forwards to libvrfhip.so (hand-written HIP kernels) -- there is no CPU path.
//
//   Rust (ark-vrf)                                         here (namespace ark_vrf_hip)
//   Secret::<S>::from_seed(seed)                           Secret<S>::from_seed(ctx, seed)
//   Secret::<S>::from_scalar(scalar)                       Secret<S>::from_scalar(ctx, scalar)
//   secret.public()                                        secret.public_key()
//   Input::<S>::new(data) -> Option<Input>                 Input<S>::new_(ctx, data) -> std::optional<Input<S>>
//   secret.output(input)                                   secret.output(ctx, input)
//   output.hash()                                          output.hash(ctx)
//   ietf::Prover::prove(&secret, input, output, ad)        ietf::prove(ctx, secret, input, output, ad)
//   ietf::Verifier::verify(&public, input, output, ad, &p) ietf::verify(ctx, public, input, output, ad, p) -> Result
//   pedersen::Prover::prove(..) -> (Proof, blinding)       pedersen::prove(..) -> std::pair<Proof, Scalar>
//   pedersen::Verifier::verify(input, output, ad, &p)      pedersen::verify(ctx, input, output, ad, p) -> Result
//   utils::te_sw_map::{te_to_sw, sw_to_te}(point)          utils::te_to_sw(ctx, points) / utils::sw_to_te(ctx, points)
//   Error::{VerificationFailure, InvalidData}              enum class Error; Result = std::optional<Error> (nullopt = Ok(()))
// Suites: the four twisted-Edwards ones (32-byte ArkworksCodec points, SHA-512), `suites::bandersnatch_sw` (33-byte
// ArkworksCodec short-Weierstrass points) and `suites::secp256r1` (33-byte Sec1
// points, big-endian scalars, SHA-256) through the same templates: Point<S> / Hash<S> carry the widths.
// Several GPUs from one process: ietf::verify_batch_sharded over one Context per device (contiguous slices, one
// host thread per context, no exchange) -- the single-process form of `bench.py --gpus N`.
// Batch forms (what the GPU is for) take std::vector of the same types: ietf::verify_batch, ietf::prove_batch,
// pedersen::verify_batch (single-MSM random-linear-combination path with automatic per-proof fallback),
// KeySet + ietf::verify_batch_keyed (public keys with HBM-resident fixed-base tables).
// Typed callers holding affine points (utils::XY) verify without compression: ietf::verify / verify_batch /
// verify_batch_sharded over ietf::ItemXY, pedersen::verify / verify_batch / verify_batch_sharded over pedersen::ItemXY.
#ifndef VRFHIP_HPP
#define VRFHIP_HPP

#include <array>
#include <cstdint>
#include <cstring>
#include <optional>
#include <random>
#include <stdexcept>
#include <string>
#include <thread>
#include <utility>
#include <vector>

#include "vrfhip.h"

namespace ark_vrf_hip {

using Bytes32 = std::array<uint8_t, 32>;
using Scalar = Bytes32;                       // `ScalarField`, 32 bytes canonical: little-endian (ArkworksCodec), big-endian on secp256r1 (Sec1Codec)
using Bytes = std::vector<uint8_t>;

// `Error` (src/lib.rs:15)
enum class Error { VerificationFailure = VRFHIP_ST_VERIFICATION_FAILURE, InvalidData = VRFHIP_ST_INVALID_DATA };
using Result = std::optional<Error>;          // std::nullopt == Ok(())

inline Result result_of(uint8_t status) {
  if (status == VRFHIP_ST_OK) return std::nullopt;
  return status == VRFHIP_ST_VERIFICATION_FAILURE ? Error::VerificationFailure : Error::InvalidData;
}

// `Suite` (src/lib.rs:16): compile-time suite tags
// POINT_LEN / HASH_LEN: bytes of an encoded point (`Suite::Codec`) and of `Output::hash()` (the suite's hash); EDWARDS:
// the twisted-Edwards suites have the key sets and the single-MSM Pedersen verifier, secp256r1 verifies per proof.
struct EdwardsSha512 {
  static constexpr size_t POINT_LEN = 32, HASH_LEN = 64;
  static constexpr bool EDWARDS = true;
};
struct BandersnatchSha512Ell2 : EdwardsSha512 {
  static constexpr vrfhip_suite ID = VRFHIP_SUITE_BANDERSNATCH_SHA512_ELL2;
  static constexpr const char* SUITE_ID = "Bandersnatch_SHA-512_ELL2";
};
struct JubJubSha512Tai : EdwardsSha512 {
  static constexpr vrfhip_suite ID = VRFHIP_SUITE_JUBJUB_SHA512_TAI;
  static constexpr const char* SUITE_ID = "JubJub_SHA-512_TAI";
};
struct Ed25519Sha512Tai : EdwardsSha512 {
  static constexpr vrfhip_suite ID = VRFHIP_SUITE_ED25519_SHA512_TAI;
  static constexpr const char* SUITE_ID = "Ed25519_SHA-512_TAI";
};
struct BabyJubJubSha512Tai : EdwardsSha512 {
  static constexpr vrfhip_suite ID = VRFHIP_SUITE_BABY_JUBJUB_SHA512_TAI;
  static constexpr const char* SUITE_ID = "BabyJubJub_SHA-512_TAI";
};
// `suites::secp256r1` (upstream "P256_SHA256_TAI", RFC 9381 ECVRF-P256-SHA256-TAI): Sec1Codec -- 33-byte compressed
// points, big-endian scalars (`Proof::c` has 16 significant bytes), SHA-256
struct Secp256r1Sha256Tai {
  static constexpr vrfhip_suite ID = VRFHIP_SUITE_SECP256R1_SHA256_TAI;
  static constexpr const char* SUITE_ID = "\x01";
  static constexpr size_t POINT_LEN = 33, HASH_LEN = 32;
  static constexpr bool EDWARDS = false;
};
// `suites::bandersnatch_sw` (upstream "Bandersnatch_SW_SHA-512_TAI"): the Bandersnatch group on its short-Weierstrass model;
// ArkworksCodec over SWAffine -- 33-byte compressed points (x little-endian, then a flag byte), little-endian scalars, SHA-512.
struct BandersnatchSwSha512Tai {
  static constexpr vrfhip_suite ID = VRFHIP_SUITE_BANDERSNATCH_SW_SHA512_TAI;
  static constexpr const char* SUITE_ID = "Bandersnatch_SW_SHA-512_TAI";
  static constexpr size_t POINT_LEN = 33, HASH_LEN = 64;
  static constexpr bool EDWARDS = false;
};
template <class S> using Point = std::array<uint8_t, S::POINT_LEN>;     // an encoded point of suite S
template <class S> using Hash = std::array<uint8_t, S::HASH_LEN>;

// API / runtime failure of the library (negative vrfhip_error): not a per-item outcome
struct ApiError : std::runtime_error {
  int code;
  ApiError(int c, const std::string& what) : std::runtime_error(what + ": " + vrfhip_last_error()), code(c) {}
};
inline void check(int32_t rc, const char* what) {
  if (rc != VRFHIP_SUCCESS) throw ApiError(rc, what);
}

// one GPU, one suite: owns the device tables and workspace
template <class S>
class Context {
 public:
  explicit Context(int device = 0) { check(vrfhip_ctx_create(S::ID, device, &h_), "vrfhip_ctx_create"); }
  // a suite given as data (`Suite::SUITE_ID`, generator, `PedersenSuite::BLINDING_BASE`, hash-to-curve DST)
  Context(const vrfhip_suite_desc& desc, int device) { check(vrfhip_ctx_create_desc(&desc, device, &h_), "vrfhip_ctx_create_desc"); }
  static vrfhip_suite_desc default_descriptor() {
    vrfhip_suite_desc d;
    check(vrfhip_suite_desc_default(S::ID, &d), "vrfhip_suite_desc_default");
    return d;
  }
  // tests only: the default descriptor with the placeholder blinding base of vrfhip_test_blinding_base (upstream's
  // `PedersenSuite::BLINDING_BASE` is pinned for Bandersnatch alone; the other default descriptors carry none)
  static vrfhip_suite_desc test_descriptor() {
    vrfhip_suite_desc d = default_descriptor();
    check(vrfhip_test_blinding_base(S::ID, d.blinding_base), "vrfhip_test_blinding_base");
    return d;
  }
  // point classes whose subgroup membership the caller vouches for (typed, already validated values):
  // VRFHIP_FLAG_PREVALIDATED_*; default 0 = arkworks' checked deserialisation inside every verify
  void set_flags(uint32_t flags) { check(vrfhip_ctx_set_flags(h_, flags), "vrfhip_ctx_set_flags"); }
  uint32_t flags() const { return vrfhip_ctx_get_flags(h_); }
  ~Context() { vrfhip_ctx_destroy(h_); }
  Context(const Context&) = delete;
  Context& operator=(const Context&) = delete;
  vrfhip_ctx* handle() const { return h_; }

 private:
  vrfhip_ctx* h_ = nullptr;
};

template <class S> struct Public { Point<S> encoded; };    // `Public`: compressed point (`Suite::Codec`)

// A set of `Public` keys whose validated points and fixed-base tables stay resident in HBM (881 KB per key):
// the verifier of a validator set builds it once and names keys by index afterwards (ietf::verify_batch_keyed).
template <class S>
class KeySet {
 public:
  KeySet(const Context<S>& ctx, const std::vector<Public<S>>& keys) : valid_(keys.size()) {
    constexpr size_t W = S::POINT_LEN;                    // every suite has key sets (secp256r1, bandersnatch_sw: round 4)
    Bytes flat(keys.size() * W), st(keys.size());
    for (size_t i = 0; i < keys.size(); ++i) std::memcpy(flat.data() + W * i, keys[i].encoded.data(), W);
    check(vrfhip_keyset_create(ctx.handle(), keys.size(), flat.data(), st.data(), &h_), "vrfhip_keyset_create");
    for (size_t i = 0; i < keys.size(); ++i) valid_[i] = st[i] == VRFHIP_ST_OK;
  }
  ~KeySet() { vrfhip_keyset_destroy(h_); }
  KeySet(const KeySet&) = delete;
  KeySet& operator=(const KeySet&) = delete;
  const vrfhip_keyset* handle() const { return h_; }
  size_t size() const { return valid_.size(); }
  bool valid(size_t i) const { return valid_[i]; }          // key i is a point of the prime-order subgroup
  size_t bytes() const { return vrfhip_keyset_bytes(h_); }

 private:
  vrfhip_keyset* h_ = nullptr;
  std::vector<bool> valid_;
};
template <class S> struct Output;

template <class S>
struct Input {                                              // `Input`
  Point<S> encoded;
  // `Input::new(data)`: hash-to-curve (Elligator 2 / try-and-increment); None never happens for these suites
  static std::optional<Input> new_(const Context<S>& ctx, const Bytes& data) {
    Input in;
    check(vrfhip_hash_to_curve_batch(ctx.handle(), 1, data.empty() ? in.encoded.data() : data.data(), nullptr,
                                     (uint32_t)data.size(), in.encoded.data()), "vrfhip_hash_to_curve_batch");
    return in;
  }
};

template <class S>
struct Output {                                             // `Output`
  Point<S> encoded;
  Hash<S> hash(const Context<S>& ctx) const {                // `Output::hash()`
    Hash<S> h;
    check(vrfhip_output_hash_batch(ctx.handle(), 1, encoded.data(), h.data()), "vrfhip_output_hash_batch");
    return h;
  }
};

template <class S>
struct Secret {                                             // `Secret`
  Scalar scalar;
  Point<S> pk;
  static Secret from_seed(const Context<S>& ctx, const Bytes& seed) {          // `Secret::from_seed`
    Secret s;
    uint8_t dummy = 0;
    check(vrfhip_secret_from_seed_batch(ctx.handle(), 1, seed.empty() ? &dummy : seed.data(), (uint32_t)seed.size(),
                                        s.scalar.data(), s.pk.data()), "vrfhip_secret_from_seed_batch");
    return s;
  }
  static Secret from_scalar(const Context<S>& ctx, const Scalar& scalar);      // `Secret::from_scalar` (throws unless scalar < order)
  Public<S> public_key() const { return Public<S>{pk}; }                       // `Secret::public`
  Output<S> output(const Context<S>& ctx, const Input<S>& in) const;           // `Secret::output`
};

namespace detail {
inline const uint8_t* ad_ptr(const Bytes& ad) {
  static const uint8_t zero = 0;
  return ad.empty() ? &zero : ad.data();
}
template <class T, class F>
Bytes column(const std::vector<T>& v, F field) {          // one field of every item, back to back (32- or 33-byte arrays)
  Bytes out;
  for (const T& t : v) {
    const auto& a = field(t);
    out.insert(out.end(), a.begin(), a.end());
  }
  if (out.empty()) out.push_back(0);
  return out;
}
template <class A>
void take(A& dst, const Bytes& flat, size_t i) { std::memcpy(dst.data(), flat.data() + dst.size() * i, dst.size()); }
}  // namespace detail

// -------------------------------------------------------------------------------- `ietf` (src/lib.rs:14)
namespace ietf {
template <class S> struct Proof { Scalar c, s; };

template <class S>
struct Item { Public<S> pub; Input<S> input; Output<S> output; Proof<S> proof; };

// `ietf::Prover::prove`
template <class S>
Proof<S> prove(const Context<S>& ctx, const Secret<S>& sk, const Input<S>& in, const Output<S>& out, const Bytes& ad) {
  Proof<S> p;
  Point<S> gamma;
  uint8_t st = 0;
  check(vrfhip_ietf_prove_batch(ctx.handle(), 1, sk.scalar.data(), nullptr, nullptr, 0, in.encoded.data(),
                                detail::ad_ptr(ad), nullptr, (uint32_t)ad.size(), gamma.data(), p.c.data(), p.s.data(),
                                nullptr, nullptr, &st), "vrfhip_ietf_prove_batch");
  if (st != VRFHIP_ST_OK || gamma != out.encoded) throw std::invalid_argument("ietf::prove: secret/input/output mismatch");
  return p;
}
// `ietf::Verifier::verify`
template <class S>
Result verify(const Context<S>& ctx, const Public<S>& pub, const Input<S>& in, const Output<S>& out, const Bytes& ad,
              const Proof<S>& p) {
  uint8_t st = 0;
  check(vrfhip_ietf_verify_batch(ctx.handle(), 1, pub.encoded.data(), in.encoded.data(), out.encoded.data(),
                                 p.c.data(), p.s.data(), detail::ad_ptr(ad), nullptr, (uint32_t)ad.size(), &st),
        "vrfhip_ietf_verify_batch");
  return result_of(st);
}
// n x verify, one launch group
template <class S>
std::vector<Result> verify_batch(const Context<S>& ctx, const std::vector<Item<S>>& items, const Bytes& ad) {
  const size_t n = items.size();
  Bytes pk = detail::column(items, [](const Item<S>& t) -> const auto& { return t.pub.encoded; });
  Bytes h = detail::column(items, [](const Item<S>& t) -> const auto& { return t.input.encoded; });
  Bytes g = detail::column(items, [](const Item<S>& t) -> const auto& { return t.output.encoded; });
  Bytes c = detail::column(items, [](const Item<S>& t) -> const auto& { return t.proof.c; });
  Bytes s = detail::column(items, [](const Item<S>& t) -> const auto& { return t.proof.s; });
  Bytes st(n);
  check(vrfhip_ietf_verify_batch(ctx.handle(), n, pk.data(), h.data(), g.data(), c.data(), s.data(), detail::ad_ptr(ad),
                                 nullptr, (uint32_t)ad.size(), st.data()), "vrfhip_ietf_verify_batch");
  std::vector<Result> r(n);
  for (size_t i = 0; i < n; ++i) r[i] = result_of(st[i]);
  return r;
}
// n x (Input::new(alpha) + verify): what a verifier holding public keys, messages and proofs runs; the inputs are hashed
// to the curve on the GPU and stay there (items[i].input is not read).
template <class S>
std::vector<Result> verify_batch_from_alpha(const Context<S>& ctx, const std::vector<Item<S>>& items,
                                            const std::vector<Bytes>& alphas, const Bytes& ad) {
  const size_t n = items.size();
  if (alphas.size() != n) throw std::invalid_argument("verify_batch_from_alpha: ragged batch");
  Bytes pk = detail::column(items, [](const Item<S>& t) -> const auto& { return t.pub.encoded; });
  Bytes g = detail::column(items, [](const Item<S>& t) -> const auto& { return t.output.encoded; });
  Bytes c = detail::column(items, [](const Item<S>& t) -> const auto& { return t.proof.c; });
  Bytes s = detail::column(items, [](const Item<S>& t) -> const auto& { return t.proof.s; });
  Bytes blob, st(n + 1);
  std::vector<uint32_t> off(n + 1, 0);
  for (size_t i = 0; i < n; ++i) { blob.insert(blob.end(), alphas[i].begin(), alphas[i].end()); off[i + 1] = (uint32_t)blob.size(); }
  blob.push_back(0);
  check(vrfhip_ietf_verify_batch_alpha(ctx.handle(), n, pk.data(), blob.data(), off.data(), 0, g.data(), c.data(), s.data(),
                                       detail::ad_ptr(ad), nullptr, (uint32_t)ad.size(), st.data()),
        "vrfhip_ietf_verify_batch_alpha");
  std::vector<Result> r(n);
  for (size_t i = 0; i < n; ++i) r[i] = result_of(st[i]);
  return r;
}
// n x verify over several contexts (one per GPU): context g verifies items [g*n/G, (g+1)*n/G) on its own host
// thread; items are independent, so the only merge is the concatenation of the results.
template <class S>
std::vector<Result> verify_batch_sharded(const std::vector<const Context<S>*>& ctxs, const std::vector<Item<S>>& items,
                                         const Bytes& ad) {
  const size_t n = items.size(), G = ctxs.size();
  if (G == 0) throw std::invalid_argument("verify_batch_sharded: no context");
  std::vector<Result> r(n);
  std::vector<std::exception_ptr> err(G);
  std::vector<std::thread> th;
  for (size_t g = 0; g < G; ++g)
    th.emplace_back([&, g] {
      try {
        const size_t lo = n * g / G, hi = n * (g + 1) / G;
        std::vector<Item<S>> part(items.begin() + lo, items.begin() + hi);
        std::vector<Result> pr = verify_batch(*ctxs[g], part, ad);
        for (size_t i = lo; i < hi; ++i) r[i] = pr[i - lo];
      } catch (...) { err[g] = std::current_exception(); }
    });
  for (auto& t : th) t.join();
  for (auto& e : err) if (e) std::rethrow_exception(e);
  return r;
}
// n x verify against keys of a KeySet: key_index[i] names the key of items[i] (items[i].pub is not read)
template <class S>
std::vector<Result> verify_batch_keyed(const Context<S>& ctx, const KeySet<S>& keys, const std::vector<uint32_t>& key_index,
                                       const std::vector<Item<S>>& items, const Bytes& ad) {
  const size_t n = items.size();
  if (key_index.size() != n) throw std::invalid_argument("verify_batch_keyed: ragged batch");
  Bytes h = detail::column(items, [](const Item<S>& t) -> const auto& { return t.input.encoded; });
  Bytes g = detail::column(items, [](const Item<S>& t) -> const auto& { return t.output.encoded; });
  Bytes c = detail::column(items, [](const Item<S>& t) -> const auto& { return t.proof.c; });
  Bytes s = detail::column(items, [](const Item<S>& t) -> const auto& { return t.proof.s; });
  Bytes st(n);
  check(vrfhip_ietf_verify_batch_keyed(ctx.handle(), keys.handle(), n, key_index.data(), h.data(), g.data(), c.data(),
                                       s.data(), detail::ad_ptr(ad), nullptr, (uint32_t)ad.size(), st.data()),
        "vrfhip_ietf_verify_batch_keyed");
  std::vector<Result> r(n);
  for (size_t i = 0; i < n; ++i) r[i] = result_of(st[i]);
  return r;
}
// n x (Input::new + Secret::output + prove) from fixed-length messages
template <class S>
std::vector<Item<S>> prove_batch(const Context<S>& ctx, const std::vector<Secret<S>>& sks, const std::vector<Bytes>& msgs,
                                 const Bytes& ad) {
  const size_t n = sks.size();
  if (msgs.size() != n) throw std::invalid_argument("prove_batch: ragged batch");
  Bytes sk = detail::column(sks, [](const Secret<S>& t) -> const auto& { return t.scalar; });
  Bytes blob;
  std::vector<uint32_t> off(n + 1, 0);
  for (size_t i = 0; i < n; ++i) { blob.insert(blob.end(), msgs[i].begin(), msgs[i].end()); off[i + 1] = (uint32_t)blob.size(); }
  blob.push_back(0);
  constexpr size_t W = S::POINT_LEN;
  Bytes g(W * n + 1), c(32 * n + 1), s(32 * n + 1), pk(W * n + 1), h(W * n + 1), st(n + 1);
  check(vrfhip_ietf_prove_batch(ctx.handle(), n, sk.data(), blob.data(), off.data(), 0, nullptr, detail::ad_ptr(ad), nullptr,
                                (uint32_t)ad.size(), g.data(), c.data(), s.data(), pk.data(), h.data(), st.data()),
        "vrfhip_ietf_prove_batch");
  std::vector<Item<S>> items(n);
  for (size_t i = 0; i < n; ++i) {
    if (st[i] != VRFHIP_ST_OK) throw std::invalid_argument("prove_batch: invalid secret");
    detail::take(items[i].pub.encoded, pk, i);
    detail::take(items[i].input.encoded, h, i);
    detail::take(items[i].output.encoded, g, i);
    detail::take(items[i].proof.c, c, i);
    detail::take(items[i].proof.s, s, i);
  }
  return items;
}
}  // namespace ietf

template <class S>
Secret<S> Secret<S>::from_scalar(const Context<S>& ctx, const Scalar& scalar) {
  Secret s;
  s.scalar = scalar;
  Point<S> gamma;
  Scalar c, sv;
  uint8_t st = 0, msg = 0;                       // the public key comes back beside a proof over a one-byte message
  check(vrfhip_ietf_prove_batch(ctx.handle(), 1, scalar.data(), &msg, nullptr, 1, nullptr, detail::ad_ptr({}), nullptr, 0,
                                gamma.data(), c.data(), sv.data(), s.pk.data(), nullptr, &st), "vrfhip_ietf_prove_batch");
  if (st != VRFHIP_ST_OK) throw std::invalid_argument("Secret::from_scalar: not a canonical scalar");
  return s;
}

template <class S>
Output<S> Secret<S>::output(const Context<S>& ctx, const Input<S>& in) const {
  Output<S> out;
  Scalar c, s;
  uint8_t st = 0;
  check(vrfhip_ietf_prove_batch(ctx.handle(), 1, scalar.data(), nullptr, nullptr, 0, in.encoded.data(), detail::ad_ptr({}),
                                nullptr, 0, out.encoded.data(), c.data(), s.data(), nullptr, nullptr, &st),
        "vrfhip_ietf_prove_batch");
  if (st != VRFHIP_ST_OK) throw std::invalid_argument("Secret::output: invalid secret or input");
  return out;
}

// -------------------------------------------------------------------------------- `pedersen` (src/lib.rs:14)
namespace pedersen {
template <class S> struct Proof { Point<S> pk_com, r, ok; Scalar s, sb; };
template <class S> struct Item { Input<S> input; Output<S> output; Proof<S> proof; };

// `pedersen::Prover::prove` -> (proof, blinding factor)
template <class S>
std::pair<Proof<S>, Scalar> prove(const Context<S>& ctx, const Secret<S>& sk, const Input<S>& in, const Output<S>& out,
                                  const Bytes& ad) {
  Proof<S> p;
  Scalar blinding;
  Point<S> gamma;
  uint8_t st = 0;
  check(vrfhip_pedersen_prove_batch(ctx.handle(), 1, sk.scalar.data(), nullptr, nullptr, 0, in.encoded.data(),
                                    detail::ad_ptr(ad), nullptr, (uint32_t)ad.size(), gamma.data(), p.pk_com.data(),
                                    p.r.data(), p.ok.data(), p.s.data(), p.sb.data(), blinding.data(), nullptr, &st),
        "vrfhip_pedersen_prove_batch");
  if (st != VRFHIP_ST_OK || gamma != out.encoded) throw std::invalid_argument("pedersen::prove: secret/input/output mismatch");
  return {p, blinding};
}
// `pedersen::Verifier::verify`
template <class S>
Result verify(const Context<S>& ctx, const Input<S>& in, const Output<S>& out, const Bytes& ad, const Proof<S>& p) {
  uint8_t st = 0;
  check(vrfhip_pedersen_verify_batch(ctx.handle(), 1, in.encoded.data(), out.encoded.data(), p.pk_com.data(), p.r.data(),
                                     p.ok.data(), p.s.data(), p.sb.data(), detail::ad_ptr(ad), nullptr, (uint32_t)ad.size(),
                                     &st), "vrfhip_pedersen_verify_batch");
  return result_of(st);
}
// n x verify through ONE multi-scalar multiplication (random linear combination); a failed batch is re-checked
// per proof inside the library, so the results are those of n calls of verify().  *fast_path (optional) tells
// whether the single MSM sufficed.  secp256r1: one launch group of per-proof checks (*fast_path = false).
template <class S>
std::vector<Result> verify_batch(const Context<S>& ctx, const std::vector<Item<S>>& items, const Bytes& ad,
                                 bool* fast_path = nullptr) {
  const size_t n = items.size();
  Bytes h = detail::column(items, [](const Item<S>& t) -> const auto& { return t.input.encoded; });
  Bytes g = detail::column(items, [](const Item<S>& t) -> const auto& { return t.output.encoded; });
  Bytes pc = detail::column(items, [](const Item<S>& t) -> const auto& { return t.proof.pk_com; });
  Bytes r = detail::column(items, [](const Item<S>& t) -> const auto& { return t.proof.r; });
  Bytes ok = detail::column(items, [](const Item<S>& t) -> const auto& { return t.proof.ok; });
  Bytes s = detail::column(items, [](const Item<S>& t) -> const auto& { return t.proof.s; });
  Bytes sb = detail::column(items, [](const Item<S>& t) -> const auto& { return t.proof.sb; });
  Bytes st(n + 1);
  int32_t fast = 1;
  {
    // every suite has the single-MSM verifier (secp256r1 since round 4)
    std::array<uint8_t, 32> seed;
    std::random_device rd;                                 // must be unpredictable to the provers
    for (auto& b : seed) b = (uint8_t)rd();
    check(vrfhip_pedersen_verify_batch_rlc(ctx.handle(), n, h.data(), g.data(), pc.data(), r.data(), ok.data(), s.data(),
                                           sb.data(), detail::ad_ptr(ad), nullptr, (uint32_t)ad.size(), seed.data(), st.data(),
                                           &fast), "vrfhip_pedersen_verify_batch_rlc");
  }
  if (fast_path) *fast_path = fast != 0;
  std::vector<Result> res(n);
  for (size_t i = 0; i < n; ++i) res[i] = result_of(st[i]);
  return res;
}
}  // namespace pedersen

// -------------------------------------------------------------------------------- `utils::te_sw_map` (src/lib.rs:14)
namespace utils {
using XY = std::array<uint8_t, 64>;           // an affine point as x || y, 32-byte little-endian canonical integers
namespace detail {
template <class S>
std::vector<std::optional<XY>> te_sw_map(const Context<S>& ctx, const std::vector<XY>& pts, int32_t to_te) {
  static_assert(S::EDWARDS || S::ID == VRFHIP_SUITE_BANDERSNATCH_SW_SHA512_TAI, "te_sw_map: the suite's curve has no twisted-Edwards model");
  const size_t n = pts.size();
  Bytes in = ark_vrf_hip::detail::column(pts, [](const XY& t) -> const XY& { return t; }), out(64 * n + 1), st(n + 1);
  check(vrfhip_te_sw_map_batch(ctx.handle(), n, to_te, in.data(), out.data(), st.data()), "vrfhip_te_sw_map_batch");
  std::vector<std::optional<XY>> r(n);
  for (size_t i = 0; i < n; ++i)
    if (st[i] == VRFHIP_ST_OK) { r[i].emplace(); ark_vrf_hip::detail::take(*r[i], out, i); }
  return r;
}
}  // namespace detail
// `te_to_sw`: points of S's twisted-Edwards curve -> the short-Weierstrass form of its Montgomery model; nullopt = None
template <class S>
std::vector<std::optional<XY>> te_to_sw(const Context<S>& ctx, const std::vector<XY>& pts) { return detail::te_sw_map(ctx, pts, 0); }
// `sw_to_te`: the inverse map
template <class S>
std::vector<std::optional<XY>> sw_to_te(const Context<S>& ctx, const std::vector<XY>& pts) { return detail::te_sw_map(ctx, pts, 1); }
}  // namespace utils

// ------------------------------------------------------- verification from affine points (typed `Public`, `Input`, `Output`)
// A caller holding arkworks values has the points as `Affine { x, y }`: utils::XY, x || y as 32-byte little-endian canonical
// integers (arkworks' in-memory Montgomery limbs on a context with VRFHIP_FLAG_COORDS_MONT256; bandersnatch_sw: the
// Weierstrass coordinates).  No point is compressed on the host and none is decompressed on the GPU; the statuses are those
// of the encoded forms above.  The *_sharded forms take one context per GPU (vrfhip_*_verify_batch_affine_multi: the
// contexts must share the suite and COORDS_MONT256).
namespace ietf {
template <class S>
struct ItemXY { utils::XY pub, input, output; Proof<S> proof; };

namespace detail_xy {
template <class S>
void columns(const std::vector<ItemXY<S>>& items, Bytes& pts, Bytes& cs) {      // pk | H | Gamma (64 B each), c | s
  const size_t n = items.size();
  pts.assign(3 * 64 * n + 1, 0);
  cs.assign(2 * 32 * n + 1, 0);
  for (size_t i = 0; i < n; ++i) {
    const ItemXY<S>& t = items[i];
    std::memcpy(pts.data() + 64 * i, t.pub.data(), 64);
    std::memcpy(pts.data() + 64 * (n + i), t.input.data(), 64);
    std::memcpy(pts.data() + 64 * (2 * n + i), t.output.data(), 64);
    std::memcpy(cs.data() + 32 * i, t.proof.c.data(), 32);
    std::memcpy(cs.data() + 32 * (n + i), t.proof.s.data(), 32);
  }
}
}  // namespace detail_xy

// `ietf::Verifier::verify` on affine points
template <class S>
Result verify(const Context<S>& ctx, const utils::XY& pub, const utils::XY& in, const utils::XY& out, const Bytes& ad,
              const Proof<S>& p) {
  uint8_t st = 0;
  check(vrfhip_ietf_verify_batch_affine(ctx.handle(), 1, pub.data(), in.data(), out.data(), p.c.data(), p.s.data(),
                                        detail::ad_ptr(ad), nullptr, (uint32_t)ad.size(), &st),
        "vrfhip_ietf_verify_batch_affine");
  return result_of(st);
}
// n x verify on affine points, one context
template <class S>
std::vector<Result> verify_batch(const Context<S>& ctx, const std::vector<ItemXY<S>>& items, const Bytes& ad) {
  const size_t n = items.size();
  Bytes pts, cs, st(n + 1);
  detail_xy::columns(items, pts, cs);
  const uint8_t* p = pts.data();
  check(vrfhip_ietf_verify_batch_affine(ctx.handle(), n, p, p + 64 * n, p + 128 * n, cs.data(), cs.data() + 32 * n,
                                        detail::ad_ptr(ad), nullptr, (uint32_t)ad.size(), st.data()),
        "vrfhip_ietf_verify_batch_affine");
  std::vector<Result> r(n);
  for (size_t i = 0; i < n; ++i) r[i] = result_of(st[i]);
  return r;
}
// n x verify on affine points over several contexts (one call: vrfhip_ietf_verify_batch_affine_multi)
template <class S>
std::vector<Result> verify_batch_sharded(const std::vector<const Context<S>*>& ctxs, const std::vector<ItemXY<S>>& items,
                                         const Bytes& ad) {
  const size_t n = items.size();
  if (ctxs.empty()) throw std::invalid_argument("verify_batch_sharded: no context");
  std::vector<vrfhip_ctx*> hs;
  for (const Context<S>* c : ctxs) hs.push_back(c->handle());
  Bytes pts, cs, st(n + 1);
  detail_xy::columns(items, pts, cs);
  const uint8_t* p = pts.data();
  check(vrfhip_ietf_verify_batch_affine_multi(hs.data(), (int32_t)hs.size(), n, p, p + 64 * n, p + 128 * n, cs.data(),
                                              cs.data() + 32 * n, detail::ad_ptr(ad), nullptr, (uint32_t)ad.size(),
                                              st.data()), "vrfhip_ietf_verify_batch_affine_multi");
  std::vector<Result> r(n);
  for (size_t i = 0; i < n; ++i) r[i] = result_of(st[i]);
  return r;
}
}  // namespace ietf

namespace pedersen {
template <class S> struct ProofXY { utils::XY pk_com, r, ok; Scalar s, sb; };
template <class S> struct ItemXY { utils::XY input, output; ProofXY<S> proof; };

namespace detail_xy {
template <class S>
void columns(const std::vector<ItemXY<S>>& items, Bytes& pts, Bytes& ss) {      // H | Gamma | pk_com | R | Ok, s | sb
  const size_t n = items.size();
  pts.assign(5 * 64 * n + 1, 0);
  ss.assign(2 * 32 * n + 1, 0);
  for (size_t i = 0; i < n; ++i) {
    const ItemXY<S>& t = items[i];
    const utils::XY* src[5] = {&t.input, &t.output, &t.proof.pk_com, &t.proof.r, &t.proof.ok};
    for (size_t k = 0; k < 5; ++k) std::memcpy(pts.data() + 64 * (k * n + i), src[k]->data(), 64);
    std::memcpy(ss.data() + 32 * i, t.proof.s.data(), 32);
    std::memcpy(ss.data() + 32 * (n + i), t.proof.sb.data(), 32);
  }
}
}  // namespace detail_xy

// `pedersen::Verifier::verify` on affine points
template <class S>
Result verify(const Context<S>& ctx, const utils::XY& in, const utils::XY& out, const Bytes& ad, const ProofXY<S>& p) {
  uint8_t st = 0;
  check(vrfhip_pedersen_verify_batch_affine(ctx.handle(), 1, in.data(), out.data(), p.pk_com.data(), p.r.data(), p.ok.data(),
                                            p.s.data(), p.sb.data(), detail::ad_ptr(ad), nullptr, (uint32_t)ad.size(), &st),
        "vrfhip_pedersen_verify_batch_affine");
  return result_of(st);
}
// n x verify on affine points, per proof, one context
template <class S>
std::vector<Result> verify_batch(const Context<S>& ctx, const std::vector<ItemXY<S>>& items, const Bytes& ad) {
  const size_t n = items.size();
  Bytes pts, ss, st(n + 1);
  detail_xy::columns(items, pts, ss);
  const uint8_t* p = pts.data();
  check(vrfhip_pedersen_verify_batch_affine(ctx.handle(), n, p, p + 64 * n, p + 128 * n, p + 192 * n, p + 256 * n, ss.data(),
                                            ss.data() + 32 * n, detail::ad_ptr(ad), nullptr, (uint32_t)ad.size(), st.data()),
        "vrfhip_pedersen_verify_batch_affine");
  std::vector<Result> r(n);
  for (size_t i = 0; i < n; ++i) r[i] = result_of(st[i]);
  return r;
}
// n x verify on affine points over several contexts (vrfhip_pedersen_verify_batch_affine_multi).  batched: one
// multi-scalar multiplication per context with the per-proof fallback, as verify_batch on encoded points
template <class S>
std::vector<Result> verify_batch_sharded(const std::vector<const Context<S>*>& ctxs, const std::vector<ItemXY<S>>& items,
                                         const Bytes& ad, bool batched = false) {
  const size_t n = items.size();
  if (ctxs.empty()) throw std::invalid_argument("verify_batch_sharded: no context");
  std::vector<vrfhip_ctx*> hs;
  for (const Context<S>* c : ctxs) hs.push_back(c->handle());
  Bytes pts, ss, st(n + 1);
  detail_xy::columns(items, pts, ss);
  std::array<uint8_t, 32> seed;
  if (batched) {
    std::random_device rd;                                 // must be unpredictable to the provers
    for (auto& b : seed) b = (uint8_t)rd();
  }
  const uint8_t* p = pts.data();
  check(vrfhip_pedersen_verify_batch_affine_multi(hs.data(), (int32_t)hs.size(), n, p, p + 64 * n, p + 128 * n, p + 192 * n,
                                                  p + 256 * n, ss.data(), ss.data() + 32 * n, detail::ad_ptr(ad), nullptr,
                                                  (uint32_t)ad.size(), batched ? seed.data() : nullptr, st.data()),
        "vrfhip_pedersen_verify_batch_affine_multi");
  std::vector<Result> r(n);
  for (size_t i = 0; i < n; ++i) r[i] = result_of(st[i]);
  return r;
}
}  // namespace pedersen

// KZG openings on BLS12-381 (`KZG10::check` / `KZG10::batch_check`): thin mirrors of vrfhip_kzg_check_batch*.  An opening is
// (commitment, point z, value v, proof) on the wire; vk = g || h || beta_h (480 bytes).  Works on a context of any suite but
// secp256r1.
namespace kzg {
struct Opening {
  std::array<uint8_t, 48> commitment;
  std::array<uint8_t, 32> point, value;
  std::array<uint8_t, 48> proof;
};
using VerifierKey = std::array<uint8_t, 480>;
namespace detail_kzg {
inline void columns(const std::vector<Opening>& items, Bytes& c, Bytes& z, Bytes& v, Bytes& pi) {
  const size_t n = items.size();
  c.resize(48 * n + 1); z.resize(32 * n + 1); v.resize(32 * n + 1); pi.resize(48 * n + 1);
  for (size_t i = 0; i < n; ++i) {
    std::memcpy(c.data() + 48 * i, items[i].commitment.data(), 48);
    std::memcpy(z.data() + 32 * i, items[i].point.data(), 32);
    std::memcpy(v.data() + 32 * i, items[i].value.data(), 32);
    std::memcpy(pi.data() + 48 * i, items[i].proof.data(), 48);
  }
}
}  // namespace detail_kzg
// n x `KZG10::check`, one pairing check per item
template <class S>
std::vector<Result> check_batch(const Context<S>& ctx, const std::vector<Opening>& items, const VerifierKey& vk) {
  const size_t n = items.size();
  Bytes c, z, v, pi, st(n + 1);
  detail_kzg::columns(items, c, z, v, pi);
  check(vrfhip_kzg_check_batch(ctx.handle(), n, c.data(), z.data(), v.data(), pi.data(), vk.data(), st.data()),
        "vrfhip_kzg_check_batch");
  std::vector<Result> r(n);
  for (size_t i = 0; i < n; ++i) r[i] = result_of(st[i]);
  return r;
}
// `KZG10::batch_check`: three multi-scalar multiplications and one pairing; a failing batch is re-checked per item, so the
// results are those of check_batch.  *batch_ok (nullable): whether the single pairing sufficed.
template <class S>
std::vector<Result> check_batch_rlc(const Context<S>& ctx, const std::vector<Opening>& items, const VerifierKey& vk,
                                    bool* batch_ok = nullptr) {
  const size_t n = items.size();
  Bytes c, z, v, pi, st(n + 1);
  detail_kzg::columns(items, c, z, v, pi);
  std::array<uint8_t, 32> seed;
  std::random_device rd;                                   // must be unpredictable to the provers
  for (auto& b : seed) b = (uint8_t)rd();
  int32_t ok = 1;
  check(vrfhip_kzg_check_batch_rlc(ctx.handle(), n, c.data(), z.data(), v.data(), pi.data(), vk.data(), seed.data(), st.data(),
                                   &ok),
        "vrfhip_kzg_check_batch_rlc");
  if (batch_ok) *batch_ok = ok != 0;
  std::vector<Result> r(n);
  for (size_t i = 0; i < n; ++i) r[i] = result_of(st[i]);
  return r;
}

// The producer side: `KZG10::commit` and the non-hiding `KZG10::open` over bases resident in HBM (vrfhip_g1_srs,
// vrfhip_kzg_commit_batch, vrfhip_kzg_open_batch).  Scalars are 32-byte little-endian integers below r.
using Scalar = std::array<uint8_t, 32>;
using G1Compressed = std::array<uint8_t, 48>;
template <class S>
class Srs {
 public:
  // throws (Error::InvalidData semantics: no set is made) if any base is not a point of the prime-order subgroup
  Srs(const Context<S>& ctx, const std::vector<G1Compressed>& bases) : n_(bases.size()) {
    Bytes flat(48 * n_ + 1);
    for (size_t i = 0; i < n_; ++i) std::memcpy(flat.data() + 48 * i, bases[i].data(), 48);
    check(vrfhip_g1_srs_create(ctx.handle(), n_, flat.data(), nullptr, &h_), "vrfhip_g1_srs_create");
  }
  ~Srs() { vrfhip_g1_srs_destroy(h_); }
  Srs(const Srs&) = delete;
  Srs& operator=(const Srs&) = delete;
  const void* handle() const { return h_; }            // the opaque vrfhip_g1_srs handle
  size_t size() const { return vrfhip_g1_srs_size(h_); }
  size_t bytes() const { return vrfhip_g1_srs_bytes(h_); }

 private:
  void* h_ = nullptr;
  size_t n_;
};
struct Commitment { G1Compressed point; Result status; };
struct OpeningProof { Scalar value; G1Compressed proof; Result status; };
namespace detail_kzg {
inline Bytes flatten(const std::vector<std::vector<Scalar>>& cols, size_t len) {
  Bytes flat(cols.size() * len * 32 + 1);
  for (size_t c = 0; c < cols.size(); ++c) {
    if (cols[c].size() != len) throw std::invalid_argument("ragged columns");
    for (size_t j = 0; j < len; ++j) std::memcpy(flat.data() + (c * len + j) * 32, cols[c][j].data(), 32);
  }
  return flat;
}
}  // namespace detail_kzg
// out[c] = sum_j columns[c][j] * srs[first + j]; all columns of one length
template <class S>
std::vector<Commitment> commit_batch(const Context<S>& ctx, const Srs<S>& srs, const std::vector<std::vector<Scalar>>& columns,
                                     size_t first = 0) {
  const size_t k = columns.size(), len = k ? columns[0].size() : 0;
  const Bytes flat = detail_kzg::flatten(columns, len);
  Bytes out(48 * k + 1), st(k + 1);
  check(vrfhip_kzg_commit_batch(ctx.handle(), srs.handle(), k, len, first, flat.data(), out.data(), nullptr, st.data()),
        "vrfhip_kzg_commit_batch");
  std::vector<Commitment> r(k);
  for (size_t c = 0; c < k; ++c) { std::memcpy(r[c].point.data(), out.data() + 48 * c, 48); r[c].status = result_of(st[c]); }
  return r;
}
// polynomial c (monomial basis) opened at points[c]: value and proof, what check_batch accepts
template <class S>
std::vector<OpeningProof> open_batch(const Context<S>& ctx, const Srs<S>& srs, const std::vector<std::vector<Scalar>>& polys,
                                     const std::vector<Scalar>& points) {
  const size_t k = polys.size(), len = k ? polys[0].size() : 0;
  if (points.size() != k) throw std::invalid_argument("one point per polynomial");
  const Bytes flat = detail_kzg::flatten(polys, len);
  Bytes z(32 * k + 1), v(32 * k + 1), out(48 * k + 1), st(k + 1);
  for (size_t c = 0; c < k; ++c) std::memcpy(z.data() + 32 * c, points[c].data(), 32);
  check(vrfhip_kzg_open_batch(ctx.handle(), srs.handle(), k, len, flat.data(), z.data(), v.data(), out.data(), nullptr,
                              st.data()),
        "vrfhip_kzg_open_batch");
  std::vector<OpeningProof> r(k);
  for (size_t c = 0; c < k; ++c) {
    std::memcpy(r[c].value.data(), v.data() + 32 * c, 32);
    std::memcpy(r[c].proof.data(), out.data() + 48 * c, 48);
    r[c].status = result_of(st[c]);
  }
  return r;
}

// Columns held as EVALUATIONS over a power-of-two domain: `Radix2EvaluationDomain` of ark-poly resident in HBM
// (vrfhip_fr_domain), its transforms (vrfhip_fr_ntt_batch), and commit / open from evaluations.
template <class S>
class Domain {
 public:
  // the plain domain of size 2^log_n
  Domain(const Context<S>& ctx, uint32_t log_n) {
    check(vrfhip_fr_domain_create(ctx.handle(), log_n, nullptr, &h_), "vrfhip_fr_domain_create");
  }
  // `get_coset(offset)`: 0 < offset < r
  Domain(const Context<S>& ctx, uint32_t log_n, const Scalar& offset) {
    check(vrfhip_fr_domain_create(ctx.handle(), log_n, offset.data(), &h_), "vrfhip_fr_domain_create");
  }
  ~Domain() { vrfhip_fr_domain_destroy(h_); }
  Domain(const Domain&) = delete;
  Domain& operator=(const Domain&) = delete;
  const void* handle() const { return h_; }            // the opaque vrfhip_fr_domain handle
  size_t size() const { return vrfhip_fr_domain_size(h_); }
  size_t bytes() const { return vrfhip_fr_domain_bytes(h_); }

 private:
  void* h_ = nullptr;
};
struct Column { std::vector<Scalar> values; Result status; };
// `fft` / `coset_fft` of every column (inverse: `ifft` / `coset_ifft`); all columns have the domain's size
template <class S>
std::vector<Column> ntt_batch(const Context<S>& ctx, const Domain<S>& dom, const std::vector<std::vector<Scalar>>& columns,
                              bool inverse = false) {
  const size_t k = columns.size(), n = dom.size();
  const Bytes flat = detail_kzg::flatten(columns, n);
  Bytes out(k * n * 32 + 1), st(k + 1);
  check(vrfhip_fr_ntt_batch(ctx.handle(), dom.handle(), k, inverse ? VRFHIP_NTT_INVERSE : 0u, flat.data(), out.data(), st.data()),
        "vrfhip_fr_ntt_batch");
  std::vector<Column> r(k);
  for (size_t c = 0; c < k; ++c) {
    r[c].values.resize(n);
    for (size_t j = 0; j < n; ++j) std::memcpy(r[c].values[j].data(), out.data() + (c * n + j) * 32, 32);
    r[c].status = result_of(st[c]);
  }
  return r;
}
// commit_batch of the polynomials that take these values over dom
template <class S>
std::vector<Commitment> commit_evals_batch(const Context<S>& ctx, const Srs<S>& srs, const Domain<S>& dom,
                                           const std::vector<std::vector<Scalar>>& evals) {
  const size_t k = evals.size();
  const Bytes flat = detail_kzg::flatten(evals, dom.size());
  Bytes out(48 * k + 1), st(k + 1);
  check(vrfhip_kzg_commit_evals_batch(ctx.handle(), srs.handle(), dom.handle(), k, flat.data(), out.data(), nullptr, st.data()),
        "vrfhip_kzg_commit_evals_batch");
  std::vector<Commitment> r(k);
  for (size_t c = 0; c < k; ++c) { std::memcpy(r[c].point.data(), out.data() + 48 * c, 48); r[c].status = result_of(st[c]); }
  return r;
}
// open_batch of the polynomials that take these values over dom, polynomial c at points[c]
template <class S>
std::vector<OpeningProof> open_evals_batch(const Context<S>& ctx, const Srs<S>& srs, const Domain<S>& dom,
                                           const std::vector<std::vector<Scalar>>& evals, const std::vector<Scalar>& points) {
  const size_t k = evals.size();
  if (points.size() != k) throw std::invalid_argument("one point per polynomial");
  const Bytes flat = detail_kzg::flatten(evals, dom.size());
  Bytes z(32 * k + 1), v(32 * k + 1), out(48 * k + 1), st(k + 1);
  for (size_t c = 0; c < k; ++c) std::memcpy(z.data() + 32 * c, points[c].data(), 32);
  check(vrfhip_kzg_open_evals_batch(ctx.handle(), srs.handle(), dom.handle(), k, flat.data(), z.data(), v.data(), out.data(),
                                    nullptr, st.data()),
        "vrfhip_kzg_open_evals_batch");
  std::vector<OpeningProof> r(k);
  for (size_t c = 0; c < k; ++c) {
    std::memcpy(r[c].value.data(), v.data() + 32 * c, 32);
    std::memcpy(r[c].proof.data(), out.data() + 48 * c, 48);
    r[c].status = result_of(st[c]);
  }
  return r;
}
}  // namespace kzg

}  // namespace ark_vrf_hip
#endif  // VRFHIP_HPP
