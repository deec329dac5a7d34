// Mutation fuzzer of the required-signer coverage core (corda_amd/csrc/cover_core.hpp)
// and of its CSR validation (csr_check.hpp check_cover), on the host, built by
// tests/test_cover_fuzz.py with g++ -fsanitize=address,undefined. A cordahip_cover
// comes from the JVM: every offset, count and token is untrusted. A bad offset or
// count must fail the batch (check_cover == the contract's ground truth); a bad
// token is data and must make its required key MALFORMED; neither may make the
// evaluator read outside a caller buffer.
//
// Every array lives in a heap block of exactly its declared entries ([n + 1]
// offsets, ntok tokens, ckey_bytes key bytes, one stack slot per token), so a
// read or write past one is an ASan report. Per round one batch is built valid
// (random threshold trees in post order over a small shared key table, 0..5
// signatures per transaction whose keys are mostly table keys), then most rounds
// mutated: an offset of tx_req_off / req_tok_off / ckey_off edited, a declared
// count (nreq, ntok, nckey, ckey_bytes) lowered, or token fields overwritten
// (nchild, weight, threshold, key: 0, 1, +-1, 2^31 - 1, 2^31, 2^32 - 1, random).
// A batch check_cover accepts is evaluated three ways -- the host workers' stack
// (LocalStack), the kernel's (SliceStack over an exact block), and, in rounds
// whose signature keys are all 32 bytes, the dense-row reader (SigKeysDense32)
// -- and every req_status, tx_status and first_missing must equal an independent
// evaluator written here: it parses the stream top-down from its last token by
// recursion (the core reduces it bottom-up with a stack), then checks
// CompositeKey.checkConstraints and fulfilment by recursion over the parsed tree.
// Exit 0 when everything matches; a sanitizer report aborts the process.
//
// usage: cover_fuzz ROUNDS RNG_SEED   (prints one JSON line of counts)
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "../corda_amd/csrc/cover_core.hpp"
#include "../corda_amd/csrc/csr_check.hpp"

using namespace cordahip;

namespace {

struct Rng {
  uint64_t s;
  uint64_t next() {  // splitmix64
    uint64_t z = (s += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
  }
  uint64_t below(uint64_t n) { return n ? next() % n : 0; }
  bool chance(uint64_t pct) { return below(100) < pct; }
};

// an exact-size heap array (an empty one is a null pointer)
template <class T>
struct Arr {
  std::unique_ptr<T[]> p;
  uint64_t n = 0;
  void make(uint64_t k) {
    n = k;
    p.reset(new T[k ? k : 1]);
    if (k) std::memset(static_cast<void*>(p.get()), 0, sizeof(T) * k);
  }
  void from(const std::vector<T>& v, uint64_t k) {  // the first k entries of v
    make(k < v.size() ? k : v.size());
    if (n) std::memcpy(static_cast<void*>(p.get()), v.data(), sizeof(T) * n);
  }
  T* get() const { return n ? p.get() : nullptr; }
};

struct SerialPar {
  template <class F>
  void operator()(uint64_t n, uint64_t, F&& fn) const {
    if (n) fn(0, n);
  }
};

void mutate_off(Rng& r, std::vector<uint64_t>& off, uint64_t limit) {
  if (off.empty()) return;
  const uint64_t i = r.below(off.size());
  uint64_t& v = off[i];
  switch (r.below(7)) {
    case 0: v = 0; break;
    case 1: v += 1 + r.below(5); break;
    case 2: v = v > 5 ? v - 1 - r.below(5) : 0; break;
    case 3: v = limit + r.below(2); break;
    case 4: v = UINT64_MAX - r.below(3); break;
    case 5: v = r.next(); break;
    default:
      if (i + 1 < off.size()) std::swap(off[i], off[i + 1]);
      break;
  }
}

// contract: off[a..b] non-decreasing and off[b] <= limit, off having n entries
bool truth(const uint64_t* off, uint64_t n, uint64_t a, uint64_t b, uint64_t limit) {
  if (b < a || b >= n) return false;
  for (uint64_t i = a; i < b; i++)
    if (off[i] > off[i + 1]) return false;
  return off[b] <= limit;
}

uint32_t odd_u32(Rng& r, uint32_t v) {
  switch (r.below(9)) {
    case 0: return 0;
    case 1: return 1;
    case 2: return v + 1;
    case 3: return v - 1;
    case 4: return 0x7fffffffu;
    case 5: return 0x80000000u;
    case 6: return 0xffffffffu;
    case 7: return (uint32_t)r.below(8);
    default: return (uint32_t)r.next();
  }
}

// a random valid tree in post order
void gen_tree(Rng& r, std::vector<cordahip_cover_tok>& out, uint32_t weight, int depth, uint32_t nckey) {
  if (depth == 0 || r.chance(45)) {
    out.push_back({0, weight, 0, (uint32_t)r.below(nckey)});
    return;
  }
  const uint32_t n = 2 + (uint32_t)r.below(3);
  uint64_t total = 0;
  for (uint32_t i = 0; i < n; i++) {
    const uint32_t w = r.chance(10) ? 0x3fffffffu : 1 + (uint32_t)r.below(5);
    total += w;
    gen_tree(r, out, w, depth - 1, nckey);
  }
  uint32_t thr = 1 + (uint32_t)r.below(total > 12 ? 12 : total);
  if (r.chance(10)) thr = (uint32_t)(total > 0x7fffffffull ? 0x7fffffffull : total);
  out.push_back({n, weight, thr, 0});
}

// ---- the independent evaluator ---------------------------------------------------
struct View {
  const cordahip_cover* c;
  const uint64_t* tx_sig_off;
  const uint8_t* scheme;
  const uint8_t* key;
  const uint64_t* key_off;
  uint64_t s0, s1;
};

struct Node {
  uint64_t tok;                // index of its token
  std::vector<uint64_t> kids;  // indices into the node pool, left to right
};

// parses the subtree whose root is token `last`, downwards; returns the index of
// its first token, or UINT64_MAX when it runs out of the range [k0, ..)
uint64_t parse(const cordahip_cover& c, uint64_t k0, uint64_t last, std::vector<Node>& pool, uint64_t& root) {
  const cordahip_cover_tok& tk = c.tok[last];
  root = pool.size();
  pool.push_back({last, {}});
  if (tk.nchild == 0) return last;
  uint64_t first = last;
  std::vector<uint64_t> kids;
  for (uint32_t i = 0; i < tk.nchild; i++) {
    if (first == k0) return UINT64_MAX;  // no token left for this child
    uint64_t kid;
    first = parse(c, k0, first - 1, pool, kid);
    if (first == UINT64_MAX) return UINT64_MAX;
    kids.push_back(kid);
    if (kids.size() > last - k0) return UINT64_MAX;
  }
  pool[root].kids.assign(kids.rbegin(), kids.rend());
  return first;
}

bool positive_int(uint32_t v) { return v >= 1 && v <= 0x7fffffffu; }

// 0 missing, 1 fulfilled, 2 malformed
int eval_node(const View& v, const std::vector<Node>& pool, uint64_t n) {
  const cordahip_cover& c = *v.c;
  const cordahip_cover_tok& tk = c.tok[pool[n].tok];
  if (tk.nchild == 0) {
    if (tk.key >= c.nckey) return 2;
    const uint64_t lo = c.ckey_off[tk.key], len = c.ckey_off[tk.key + 1] - lo;
    for (uint64_t s = v.s0; s < v.s1; s++)
      if (v.scheme[s] == c.ckey_scheme[tk.key] && v.key_off[s + 1] - v.key_off[s] == len &&
          (len == 0 || std::memcmp(v.key + v.key_off[s], c.ckey + lo, len) == 0))
        return 1;
    return 0;
  }
  if (tk.nchild < 2 || !positive_int(tk.threshold)) return 2;
  int64_t total = 0, got = 0;
  bool bad = false;
  for (uint64_t kid : pool[n].kids) {
    const uint32_t w = c.tok[pool[kid].tok].weight;
    if (!positive_int(w)) bad = true;
    total += w;
    const int f = eval_node(v, pool, kid);
    if (f == 2) bad = true;
    if (f == 1) got += w;
  }
  if (bad || total > 0x7fffffffll || (int64_t)tk.threshold > total) return 2;
  return got >= (int64_t)tk.threshold ? 1 : 0;
}

uint8_t ref_req(const View& v, uint64_t r) {
  const cordahip_cover& c = *v.c;
  const uint64_t k0 = c.req_tok_off[r], k1 = c.req_tok_off[r + 1];
  if (k0 == k1) return CORDAHIP_REQ_MALFORMED;
  std::vector<Node> pool;
  uint64_t root;
  if (parse(c, k0, k1 - 1, pool, root) != k0) return CORDAHIP_REQ_MALFORMED;  // not exactly one tree
  const int f = eval_node(v, pool, root);
  return f == 2 ? CORDAHIP_REQ_MALFORMED : f == 1 ? CORDAHIP_REQ_FULFILLED : CORDAHIP_REQ_MISSING;
}

struct Stats {
  uint64_t batches = 0, invalid = 0, txs = 0, dense_batches = 0;
  uint64_t req[5] = {0, 0, 0, 0, 0};
  uint64_t tx_ok = 0, tx_missing = 0, tx_bad_cover = 0, tx_kept = 0;
};

bool round(Rng& r, Stats& st) {
  const uint64_t ntx = r.below(24);
  const bool dense = r.chance(30);  // every signature key 32 bytes: also through SigKeysDense32
  // the key table: a few keys, some sharing their bytes under another scheme
  const uint32_t nckey = 1 + (uint32_t)r.below(8);
  std::vector<uint8_t> ckey_scheme, ckey;
  std::vector<uint64_t> ckey_off{0};
  for (uint32_t k = 0; k < nckey; k++) {
    const uint64_t len = r.chance(60) ? 32 : r.chance(50) ? 33 : r.below(41);
    ckey_scheme.push_back((uint8_t)(1 + r.below(5)));
    if (k && r.chance(25) && ckey_off[k] - ckey_off[k - 1] == len) {  // the previous key's bytes again
      for (uint64_t i = 0; i < len; i++) ckey.push_back(ckey[ckey_off[k - 1] + i]);
    } else {
      for (uint64_t i = 0; i < len; i++) ckey.push_back((uint8_t)r.below(3));
    }
    ckey_off.push_back(ckey.size());
  }
  // transactions: required keys and signatures
  std::vector<uint64_t> tx_req_off{0}, req_tok_off{0}, tx_sig_off{0}, key_off{0};
  std::vector<cordahip_cover_tok> tok;
  std::vector<uint8_t> req_flags, scheme, key, tx_status;
  for (uint64_t t = 0; t < ntx; t++) {
    const uint64_t nr = r.below(4);
    for (uint64_t q = 0; q < nr; q++) {
      if (!r.chance(3)) gen_tree(r, tok, (uint32_t)r.below(3), 3, nckey);  // else an empty token range
      req_tok_off.push_back(tok.size());
      req_flags.push_back((uint8_t)(r.chance(20) ? 1 + 2 * r.below(2) : 2 * r.below(2)));
    }
    tx_req_off.push_back(req_flags.size());
    const uint64_t ns = r.below(6);
    for (uint64_t q = 0; q < ns; q++) {
      const uint32_t k = (uint32_t)r.below(nckey);
      uint64_t len = ckey_off[k + 1] - ckey_off[k];
      scheme.push_back(r.chance(85) ? ckey_scheme[k] : (uint8_t)(1 + r.below(5)));
      if (dense && len != 32) {
        len = 32;
        for (uint64_t i = 0; i < len; i++) key.push_back((uint8_t)r.below(3));
      } else {
        for (uint64_t i = 0; i < len; i++) key.push_back(ckey[ckey_off[k] + i]);
        if (len && r.chance(10)) key.back() ^= 1;
      }
      key_off.push_back(key.size());
    }
    tx_sig_off.push_back(scheme.size());
    tx_status.push_back(r.chance(85) ? 0 : (uint8_t)(1 + r.below(9)));
  }
  // mutations and the library's view: arrays of exactly the declared entries
  uint64_t nreq = req_flags.size(), ntok = tok.size(), nck = nckey, ckb = ckey.size();
  if (r.chance(70)) {
    switch (r.below(9)) {
      case 0: mutate_off(r, tx_req_off, nreq); break;
      case 1: mutate_off(r, req_tok_off, ntok); break;
      case 2: mutate_off(r, ckey_off, ckb); break;
      case 3: nreq = nreq ? nreq - 1 - r.below(nreq < 3 ? nreq : 3) : 0; break;
      case 4: ntok = ntok ? ntok - 1 - r.below(ntok < 3 ? ntok : 3) : 0; break;
      case 5: nck = nck - 1 - r.below(nck < 3 ? nck : 3); break;
      case 6: ckb = ckb ? ckb - 1 - r.below(ckb < 40 ? ckb : 40) : 0; break;
      default:  // token contents: the CSR stays valid, trees go bad
        for (uint64_t m = 1 + r.below(4); m && !tok.empty(); m--) {
          cordahip_cover_tok& tk = tok[r.below(tok.size())];
          switch (r.below(4)) {
            case 0: tk.nchild = odd_u32(r, tk.nchild); break;
            case 1: tk.weight = odd_u32(r, tk.weight); break;
            case 2: tk.threshold = odd_u32(r, tk.threshold); break;
            default: tk.key = odd_u32(r, tk.key); break;
          }
        }
        break;
    }
  }
  Arr<uint64_t> a_tx_req_off, a_req_tok_off, a_ckey_off, a_tx_sig_off, a_key_off, a_stack;
  Arr<cordahip_cover_tok> a_tok;
  Arr<uint8_t> a_flags, a_cscheme, a_ckey, a_req_status, a_scheme, a_key, a_status;
  Arr<int64_t> a_first;
  a_tx_req_off.from(tx_req_off, ntx + 1);
  a_req_tok_off.from(req_tok_off, nreq + 1);
  a_tok.from(tok, ntok);
  a_flags.from(req_flags, nreq);
  a_cscheme.from(ckey_scheme, nck);
  a_ckey.from(ckey, ckb);
  a_ckey_off.from(ckey_off, nck + 1);
  a_req_status.make(nreq);
  a_first.make(ntx);
  a_tx_sig_off.from(tx_sig_off, ntx + 1);
  a_scheme.from(scheme, scheme.size());
  a_key.from(key, key.size());
  a_key_off.from(key_off, key_off.size());
  const bool no_flags = r.chance(15);
  const cordahip_cover c{a_tx_req_off.get(), a_req_tok_off.get(), a_tok.get(), no_flags ? nullptr : a_flags.get(),
                         a_cscheme.get(), a_ckey.get(), a_ckey_off.get(), a_req_status.get(), a_first.get(),
                         nreq, ntok, nck, ckb};
  // the contract's ground truth (include/cordahip.h, csr_check.hpp check_cover)
  bool valid = true;
  if (ntx) {
    valid = truth(tx_req_off.data(), ntx + 1, 0, ntx, nreq);
    if (valid && tx_req_off[0] != tx_req_off[ntx]) {
      valid = truth(req_tok_off.data(), nreq + 1, tx_req_off[0], tx_req_off[ntx], ntok);
      if (valid && nck) valid = truth(ckey_off.data(), nck + 1, 0, nck, ckb);
    }
  }
  const bool ok = rt::check_cover(SerialPar{}, &c, ntx);
  st.batches++;
  st.invalid += !ok;
  if (ok != valid) {
    fprintf(stderr, "cover: check_cover says %s, the contract %s (ntx %llu)\n", ok ? "valid" : "invalid",
            valid ? "valid" : "invalid", (unsigned long long)ntx);
    return false;
  }
  if (!ok || !ntx) return true;
  // the reference verdicts
  std::vector<uint8_t> want_req(nreq, 0xee), want_status(tx_status);
  std::vector<int64_t> want_first(ntx, -1);
  for (uint64_t t = 0; t < ntx; t++) {
    const uint64_t r0 = tx_req_off[t], r1 = tx_req_off[t + 1];
    if (tx_status[t] != 0) {
      for (uint64_t q = r0; q < r1; q++) want_req[q] = CORDAHIP_REQ_NOT_EVALUATED;
      continue;
    }
    const View v{&c, a_tx_sig_off.get(), a_scheme.get(), a_key.get(), a_key_off.get(), tx_sig_off[t], tx_sig_off[t + 1]};
    int64_t mal = -1, miss = -1;
    for (uint64_t q = r0; q < r1; q++) {
      uint8_t s = ref_req(v, q);
      if (s == CORDAHIP_REQ_MISSING && !no_flags && (req_flags[q] & 1)) s = CORDAHIP_REQ_MISSING_ALLOWED;
      want_req[q] = s;
      if (s == CORDAHIP_REQ_MALFORMED && mal < 0) mal = (int64_t)(q - r0);
      if (s == CORDAHIP_REQ_MISSING && miss < 0) miss = (int64_t)(q - r0);
    }
    if (mal >= 0) want_status[t] = CORDAHIP_TX_BAD_COVER, want_first[t] = mal;
    else if (miss >= 0) want_status[t] = CORDAHIP_TX_SIGNATURES_MISSING, want_first[t] = miss;
  }
  // the core, every way it is used
  const int nways = dense ? 3 : 2;
  for (int way = 0; way < nways; way++) {
    a_status.from(tx_status, ntx);
    std::memset(a_req_status.p.get(), 0xdd, nreq);
    for (uint64_t t = 0; t < ntx; t++) a_first.p[t] = -77;
    const cover::SigKeysCsr csr{a_scheme.get(), a_key.get(), a_key_off.get()};
    if (way == 0) {
      cover::LocalStack stack;
      for (uint64_t t = 0; t < ntx; t++) cover::tx_eval(c, t, a_status.get(), a_tx_sig_off.get(), csr, stack);
      if (stack.failed) return false;
    } else {
      a_stack.make(ntok);  // one slot per token, exactly
      cover::SliceStack stack{a_stack.get()};
      if (way == 1) {
        for (uint64_t t = 0; t < ntx; t++) cover::tx_eval(c, t, a_status.get(), a_tx_sig_off.get(), csr, stack);
      } else {
        const cover::SigKeysDense32 rows{a_scheme.get(), a_key.get()};  // operator new[]: 16-byte aligned
        for (uint64_t t = 0; t < ntx; t++) cover::tx_eval(c, t, a_status.get(), a_tx_sig_off.get(), rows, stack);
      }
    }
    for (uint64_t t = 0; t < ntx; t++) {
      bool same = a_status.p[t] == want_status[t] && a_first.p[t] == want_first[t];
      for (uint64_t q = tx_req_off[t]; q < tx_req_off[t + 1]; q++) same = same && a_req_status.p[q] == want_req[q];
      if (!same) {
        fprintf(stderr, "cover: way %d, tx %llu: status %u first %lld, the reference %u / %lld\n", way,
                (unsigned long long)t, a_status.p[t], (long long)a_first.p[t], want_status[t], (long long)want_first[t]);
        return false;
      }
    }
  }
  st.dense_batches += dense;
  for (uint64_t t = 0; t < ntx; t++) {
    st.txs++;
    if (tx_status[t] != 0) st.tx_kept++;
    else if (want_status[t] == 0) st.tx_ok++;
    else if (want_status[t] == CORDAHIP_TX_BAD_COVER) st.tx_bad_cover++;
    else st.tx_missing++;
    for (uint64_t q = tx_req_off[t]; q < tx_req_off[t + 1]; q++) st.req[want_req[q]]++;
  }
  return true;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc < 3) {
    fprintf(stderr, "usage: cover_fuzz ROUNDS RNG_SEED\n");
    return 2;
  }
  const uint64_t rounds = strtoull(argv[1], nullptr, 10);
  Rng r{strtoull(argv[2], nullptr, 10)};
  Stats st;
  for (uint64_t k = 0; k < rounds; k++)
    if (!round(r, st)) return 1;
  printf("{\"rounds\": %llu, \"batches\": %llu, \"invalid\": %llu, \"dense_batches\": %llu, \"txs\": %llu, "
         "\"tx_ok\": %llu, \"tx_missing\": %llu, \"tx_bad_cover\": %llu, \"tx_kept\": %llu, "
         "\"req_fulfilled\": %llu, \"req_missing\": %llu, \"req_allowed\": %llu, \"req_not_evaluated\": %llu, "
         "\"req_malformed\": %llu}\n",
         (unsigned long long)rounds, (unsigned long long)st.batches, (unsigned long long)st.invalid,
         (unsigned long long)st.dense_batches, (unsigned long long)st.txs, (unsigned long long)st.tx_ok,
         (unsigned long long)st.tx_missing, (unsigned long long)st.tx_bad_cover, (unsigned long long)st.tx_kept,
         (unsigned long long)st.req[0], (unsigned long long)st.req[1], (unsigned long long)st.req[2],
         (unsigned long long)st.req[3], (unsigned long long)st.req[4]);
  return 0;
}
