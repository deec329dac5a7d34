"""RSA_SHA256 (RSASSA-PSS) on the CPU: the restatement (tests/golden/bc_rsa_pss.py) against
the recorded golden statuses and against OpenSSL, and the library's host code
(corda_amd/csrc/rsa_key.hpp: strict key parser, width-class rule, word-serial Montgomery
modexp, the whole reference verification) against the restatement on the goldens and on a
few thousand mutated keys and signatures -- once through a g++-built harness loaded here,
once as a stand-alone program built with -fsanitize=address,undefined and run as a
subprocess."""
import ctypes
import json
import os
import random
import struct
import subprocess

import pytest

from conftest import ROOT

import bc_rsa_pss as bc

try:
    import openssl_rsa_pss as ossl
    ossl.lib()
except (OSError, AttributeError) as exc:  # no libcrypto 3 on this machine
    pytest.skip("OpenSSL libcrypto cannot be loaded: %s" % exc, allow_module_level=True)

CSRC = os.path.join(ROOT, "corda_amd", "csrc")

HARNESS = r'''
#include <stdint.h>
#include <string.h>
#include "rsa_key.hpp"
using namespace cordahip;
extern "C" int rsa_parse(const uint8_t* der, uint64_t len, uint32_t* n /* [128] */, uint32_t* meta /* e, bits, words */) {
  rsa::PublicKey pk;
  const uint8_t st = rsa::parse_public_key(der, len, pk);
  if (st != rsa::kOk) return st;
  memcpy(n, pk.n, sizeof(pk.n));
  meta[0] = pk.e, meta[1] = pk.bits, meta[2] = pk.words;
  return 0;
}
extern "C" int rsa_verify(const uint8_t* key, uint64_t kl, const uint8_t* sig, uint64_t sl, const uint8_t* msg,
                          uint64_t ml, int do_verify) {
  return rsa::verify(key, kl, sig, sl, msg, ml, do_verify != 0);
}
extern "C" int rsa_modexp(const uint32_t* n, uint32_t e, const uint32_t* in, uint32_t w, uint32_t* out) {
  return rsa::modexp(n, e, in, w, out) ? 1 : 0;
}
extern "C" void rsa_mont_mul(const uint32_t* a, const uint32_t* b, const uint32_t* n, uint32_t w, uint32_t* out) {
  rsa::mont_mul(a, b, n, rsa::mont_nprime(n[0]), w, out);
}
extern "C" uint32_t rsa_class_words(uint32_t bits) { return rsa::class_words(bits); }
'''

# reads records (u32 key_len, sig_len, msg_len, do_verify, want; then the bytes) and checks each
SAN_MAIN = r'''
#include <stdint.h>
#include <stdio.h>
#include <vector>
#include "rsa_key.hpp"
int main(int argc, char** argv) {
  if (argc < 2) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  uint32_t h[5];
  unsigned long cases = 0, bad = 0;
  while (fread(h, 4, 5, f) == 5) {
    std::vector<uint8_t> key(h[0]), sig(h[1]), msg(h[2]);
    if ((h[0] && fread(key.data(), 1, h[0], f) != h[0]) || (h[1] && fread(sig.data(), 1, h[1], f) != h[1]) ||
        (h[2] && fread(msg.data(), 1, h[2], f) != h[2]))
      return 2;
    const uint8_t got = cordahip::rsa::verify(key.data(), h[0], sig.data(), h[1], msg.data(), h[2], h[3] != 0);
    if (got != h[4]) {
      if (bad++ < 10) fprintf(stderr, "case %lu: got %u want %u\n", cases, got, h[4]);
    }
    cases++;
  }
  fclose(f);
  printf("%lu cases, %lu mismatches\n", cases, bad);
  return bad ? 1 : 0;
}
'''


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(ROOT, "tests", "golden", "rsa_pss_vectors.json")) as f:
        g = json.load(f)
    keys = [bytes.fromhex(k["der"]) for k in g["keys"]]
    vs = [dict(v, der=keys[v["key"]], sig=bytes.fromhex(v["sig"]), msg=bytes.fromhex(v["msg"])) for v in g["vectors"]]
    return g["keys"], vs


@pytest.fixture(scope="module")
def mutants(golden):
    """(key, sig, msg) triples: golden vectors with a mutated key or signature."""
    _, vs = golden
    rng = random.Random(0x5A17)
    base = [v for v in vs if v["cat"] in ("valid", "valid_openssl", "top_bit", "stripped_leading_zero", "declined_key_valid")]
    out = []
    for t in range(3000):
        v = rng.choice(base)
        key, sig = bytearray(v["der"]), bytearray(v["sig"])
        tgt = key if t % 3 == 0 else sig
        op = rng.randrange(6)
        if op == 0:
            tgt[rng.randrange(len(tgt))] ^= 1 << rng.randrange(8)
        elif op == 1:
            del tgt[rng.randrange(len(tgt)):]
        elif op == 2:
            tgt.insert(rng.randrange(len(tgt) + 1), rng.randrange(256))
        elif op == 3:
            tgt[rng.randrange(min(8, len(tgt)))] = rng.randrange(256)  # the DER header / the top bytes
        elif op == 4:
            tgt[-1 - rng.randrange(min(6, len(tgt)))] ^= 1 << rng.randrange(8)  # the exponent / the low bytes
        else:
            tgt += bytes([rng.randrange(256)])
        out.append((bytes(key), bytes(sig), v["msg"] if t % 7 else b""))
    return out


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    d = tmp_path_factory.mktemp("rsa")
    src, so = d / "rsa_probe.cpp", d / "rsa_probe.so"
    src.write_text(HARNESS)
    subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-I", CSRC, "-o", str(so),
                    str(src)], check=True)
    l = ctypes.CDLL(str(so))
    cp, u64, u32, vp = ctypes.c_char_p, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_void_p
    l.rsa_parse.argtypes = [cp, u64, vp, vp]
    l.rsa_verify.argtypes = [cp, u64, cp, u64, cp, u64, ctypes.c_int]
    l.rsa_modexp.argtypes = [vp, u32, vp, u32, vp]
    l.rsa_mont_mul.argtypes = [vp, vp, vp, u32, vp]
    l.rsa_class_words.argtypes = [u32]
    l.rsa_class_words.restype = u32
    return l


def words(x, w):
    return (ctypes.c_uint32 * w)(*[(x >> (32 * i)) & 0xFFFFFFFF for i in range(w)])


def number(arr):
    return sum(int(v) << (32 * i) for i, v in enumerate(arr))


def test_restatement_gives_the_recorded_statuses(golden):
    keys, vs = golden
    assert len(vs) > 150 and len(keys) >= 12
    cats = {v["cat"] for v in vs}
    for c in ("valid_openssl", "wrong_message", "wrong_key", "bit_flip", "s_edge", "leading_zero_k_plus_1",
              "stripped_leading_zero", "trailer", "salt_len_0", "salt_len_20", "nonzero_padding", "m_above_em",
              "top_bit", "empty_signature", "empty_message", "declined_key", "malformed_key"):
        assert c in cats, c
    for v in vs:
        assert bc.verify(v["der"], v["sig"], v["msg"]) == v["status"], v["cat"]
        assert bc.verify(v["der"], v["sig"], v["msg"], is_valid=True) == v["status_is_valid"], v["cat"]
    # what the categories are for
    for v in vs:
        if v["cat"] in ("valid", "valid_openssl", "top_bit", "stripped_leading_zero"):
            assert v["status"] == bc.OK, v["cat"]
        elif v["cat"] in ("declined_key", "declined_key_valid"):
            assert v["status"] == v["status_is_valid"] == bc.UNSUPPORTED
        elif v["cat"].startswith("malformed_key"):
            assert v["status"] == v["status_is_valid"] == bc.BAD_KEY
        elif v["cat"] in ("empty_signature", "empty_message"):
            assert v["status"] == bc.EMPTY
            assert v["status_is_valid"] == (bc.OK if v["cat"] == "empty_message" else bc.BAD_SIG)
        else:
            assert v["status"] == v["status_is_valid"] == bc.BAD_SIG, v["cat"]


def test_restatement_agrees_with_openssl(golden):
    """Every vector whose key OpenSSL accepts, except the top_bit category (BC clears the unused
    bits of DB[0] without checking them in EM; OpenSSL checks): as many exceptions as top_bit
    vectors, nothing else skipped."""
    _, vs = golden
    exceptions = 0
    for v in vs:
        got = ossl.verify(v["der"], v["sig"], v["msg"])
        if got is None:
            assert bc.decode_key(v["der"], decline=False) == bc.BAD_KEY, v["cat"]
            continue
        want = bc.verify(v["der"], v["sig"], v["msg"], is_valid=True, decline=False) == bc.OK
        if v["cat"] == "top_bit":
            assert want and not got
            exceptions += 1
        else:
            assert got == want, v["cat"]
    assert exceptions == sum(v["cat"] == "top_bit" for v in vs) > 0


def test_host_parser_and_class_rule(harness, golden, mutants):
    keys, vs = golden
    ders = [bytes.fromhex(k["der"]) for k in keys] + [m[0] for m in mutants]
    seen = set()
    for der in ders:
        n = (ctypes.c_uint32 * 128)()
        meta = (ctypes.c_uint32 * 3)()
        st = harness.rsa_parse(der, len(der), n, meta)
        want = bc.decode_key(der)
        seen.add(st)
        if isinstance(want, int):
            assert st == want, der.hex()[:80]
            continue
        assert st == 0
        bits = want[0].bit_length()
        assert (number(n), meta[0], meta[1]) == (want[0], want[1], bits)
        assert meta[2] == (64 if bits <= 2048 else 96 if bits <= 3072 else 128)
    assert seen == {bc.OK, bc.BAD_KEY, bc.UNSUPPORTED}
    for bits, w in ((1023, 0), (1024, 64), (2048, 64), (2049, 96), (3072, 96), (3073, 128), (4096, 128), (4097, 0)):
        assert harness.rsa_class_words(bits) == w


def test_host_reference_verification(harness, golden, mutants):
    _, vs = golden
    for v in vs:
        for is_valid, name in ((False, "status"), (True, "status_is_valid")):
            got = harness.rsa_verify(v["der"], len(v["der"]), v["sig"], len(v["sig"]), v["msg"], len(v["msg"]),
                                     0 if is_valid else 1)
            assert got == v[name], (v["cat"], name)
    hist = {}
    for t, (key, sig, msg) in enumerate(mutants):
        want = bc.verify(key, sig, msg, is_valid=bool(t & 1))
        got = harness.rsa_verify(key, len(key), sig, len(sig), msg, len(msg), 0 if t & 1 else 1)
        assert got == want, (t, key.hex()[:40])
        hist[want] = hist.get(want, 0) + 1
    assert set(hist) >= {bc.OK, bc.BAD_SIG, bc.BAD_KEY, bc.UNSUPPORTED, bc.EMPTY}, hist


@pytest.mark.parametrize("w", (64, 96, 128))
def test_host_montgomery_against_pow(harness, w):
    rng = random.Random(w)
    r = 1 << (32 * w)
    mods = [r - 1, (1 << (32 * w - 1)) + 1, (rng.getrandbits(32 * w - 97) << 96) | ((1 << 96) - 1) | (1 << (32 * w - 1)),
            rng.getrandbits(32 * w) | 1 | (1 << (32 * w - 1)), rng.getrandbits(32 * w - 1000) | 1]
    for n in mods:
        rinv = pow(r, -1, n)
        for a, b in ((n - 1, n - 1), (0, n - 1), (1, 1), (rng.randrange(n), rng.randrange(n))):
            out = (ctypes.c_uint32 * w)()
            harness.rsa_mont_mul(words(a, w), words(b, w), words(n, w), w, out)
            assert number(out) == a * b * rinv % n
        for a in (n - 1, 0, 1, rng.randrange(n)):
            for e in (1, 3, 65537, (1 << 32) - 1):
                out = (ctypes.c_uint32 * w)()
                assert harness.rsa_modexp(words(n, w), e, words(a, w), w, out) == 1
                assert number(out) == pow(a, e, n), (w, hex(n)[:20], a, e)
    # the contract: even modulus, e = 0, in >= n give a zero row
    n = mods[3]
    for nn, e, a in ((n + 1, 3, 5), (n, 0, 5), (n, 3, n), (n, 3, n + 2)):
        out = (ctypes.c_uint32 * w)(*([7] * w))
        assert harness.rsa_modexp(words(nn, w), e, words(a, w), w, out) == 0 and number(out) == 0


def test_sanitized_standalone_program(tmp_path, golden, mutants):
    """rsa_key.hpp under AddressSanitizer and UBSan in a program of its own (nothing sanitized
    is loaded into this process): the goldens under both flag values and the mutants."""
    _, vs = golden
    src, exe, corpus = tmp_path / "rsa_san.cpp", tmp_path / "rsa_san", tmp_path / "corpus.bin"
    src.write_text(SAN_MAIN)
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", CSRC, "-o", str(exe), str(src)], check=True)
    n = 0
    with open(corpus, "wb") as f:
        def put(key, sig, msg, do_verify):
            f.write(struct.pack("<5I", len(key), len(sig), len(msg), do_verify,
                                bc.verify(key, sig, msg, is_valid=not do_verify)))
            f.write(key + sig + msg)
        for v in vs:
            for do_verify in (1, 0):
                put(v["der"], v["sig"], v["msg"], do_verify)
                n += 1
        for t, (key, sig, msg) in enumerate(mutants):
            put(key, sig, msg, t & 1)
            n += 1
    r = subprocess.run([str(exe), str(corpus)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("%d cases, 0 mismatches" % n), r.stdout
