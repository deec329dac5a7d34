"""Pure-Python restatement of the RSA_SHA256 lane (Crypto.kt:77-88,
"SHA256WITHRSAANDMGF1" on BouncyCastle 1.57: PSSSignatureSpi -> PSSSigner.verifySignature
over RSABlindedEngine / RSACoreEngine): RSASSA-PSS with SHA-256, MGF1-SHA-256, salt
length 32, trailer 0xBC, and the library's rules for the key's wire form (the SPKI BIT
STRING payload, DER RSAPublicKey).

PARITY UNPINNED: the BouncyCastle sources are not available to this repository and the
reference holds no RSA signature, so the edge rules below are restated from BC 1.57 as
published. The happy path and every rule OpenSSL shares are pinned by the local libcrypto
(openssl_rsa_pss.py); the one rule known to differ is `top_bit`: BC clears the unused top
bits of DB[0] after unmasking and never checks that they were zero in EM (RFC 8017
9.1.2 step 6, which OpenSSL enforces).

Statuses are the library's (include/cordahip.h)."""
import hashlib

OK, BAD_SIG, MALFORMED_SIG, BAD_KEY, UNSUPPORTED, EMPTY = 0, 1, 2, 3, 4, 5
SALT_LEN = 32


def _der_len(b: bytes, i: int):
    """(length, next index) of a definite, minimal DER length at b[i], or None."""
    if i >= len(b):
        return None
    l0 = b[i]
    i += 1
    if l0 < 0x80:
        return l0, i
    nb = l0 & 0x7F
    if nb == 0 or nb > 4 or i + nb > len(b) or b[i] == 0:
        return None
    v = int.from_bytes(b[i:i + nb], "big")
    if v < 0x80:
        return None
    return v, i + nb


def _der_int(b: bytes, i: int):
    """(value, next index) of a strict DER INTEGER at b[i], or None."""
    if i >= len(b) or b[i] != 0x02:
        return None
    r = _der_len(b, i + 1)
    if r is None:
        return None
    l, i = r
    if l == 0 or i + l > len(b):
        return None
    body = b[i:i + l]
    if l > 1 and ((body[0] == 0 and body[1] < 0x80) or (body[0] == 0xFF and body[1] >= 0x80)):
        return None
    return int.from_bytes(body, "big", signed=True), i + l


def decode_key(der: bytes, decline: bool = True):
    """RSAPublicKey ::= SEQUENCE { modulus INTEGER, publicExponent INTEGER } -> (n, e), or a
    status: BAD_KEY (not exactly that, or n <= 0 / e <= 0), UNSUPPORTED (a key BC accepts and
    the GPU path declines: even n, bits outside 1024..4096, even e, e < 3, e >= 2^32).
    decline=False: BouncyCastle's own view, which keeps those keys."""
    if len(der) < 2 or der[0] != 0x30:
        return BAD_KEY
    r = _der_len(der, 1)
    if r is None or r[1] + r[0] != len(der):
        return BAD_KEY
    i = r[1]
    a = _der_int(der, i)
    if a is None:
        return BAD_KEY
    c = _der_int(der, a[1])
    if c is None or c[1] != len(der):
        return BAD_KEY
    n, e = a[0], c[0]
    if n <= 0 or e <= 0:
        return BAD_KEY
    if decline and (n % 2 == 0 or not 1024 <= n.bit_length() <= 4096 or e % 2 == 0 or e < 3 or e >= 1 << 32):
        return UNSUPPORTED
    return n, e


def encode_key(n: int, e: int) -> bytes:
    def integer(x):
        body = x.to_bytes(x.bit_length() // 8 + 1, "big", signed=True)
        return b"\x02" + length(len(body)) + body

    def length(l):
        if l < 0x80:
            return bytes([l])
        lb = l.to_bytes((l.bit_length() + 7) // 8, "big")
        return bytes([0x80 | len(lb)]) + lb
    content = integer(n) + integer(e)
    return b"\x30" + length(len(content)) + content


def mgf1(seed: bytes, n: int) -> bytes:
    out = b""
    ctr = 0
    while len(out) < n:
        out += hashlib.sha256(seed + ctr.to_bytes(4, "big")).digest()
        ctr += 1
    return out[:n]


def pss_check(m: int, bits: int, msg: bytes) -> bool:
    """Rules 3-8 on m = s^e mod n."""
    em_bits = bits - 1
    em_len = (em_bits + 7) // 8
    if m >= 1 << (8 * em_len):
        return False
    em = m.to_bytes(em_len, "big")
    if em[-1] != 0xBC:
        return False
    db_len = em_len - 33
    h = em[db_len:db_len + 32]
    db = bytearray(x ^ y for x, y in zip(em[:db_len], mgf1(h, db_len)))
    db[0] &= 0xFF >> (8 * em_len - em_bits)  # cleared, never checked
    if any(db[:db_len - SALT_LEN - 1]) or db[db_len - SALT_LEN - 1] != 0x01:
        return False
    salt = bytes(db[db_len - SALT_LEN:])
    return hashlib.sha256(bytes(8) + hashlib.sha256(msg).digest() + salt).digest() == h


def verify(key: bytes, sig: bytes, msg: bytes, is_valid: bool = False, decline: bool = True) -> int:
    """The lane's status; precedence UNSUPPORTED > BAD_KEY > EMPTY > the checks.
    decline=False: what BouncyCastle says of the keys the GPU path leaves to the JVM."""
    k = decode_key(key, decline)
    if isinstance(k, int):
        return k
    n, e = k
    if not is_valid and (len(sig) == 0 or len(msg) == 0):
        return EMPTY
    if len(sig) > (n.bit_length() + 7) // 8:
        return BAD_SIG
    s = int.from_bytes(sig, "big")
    if s >= n:
        return BAD_SIG
    return OK if pss_check(pow(s, e, n), n.bit_length(), msg) else BAD_SIG


def encode_em(msg: bytes, bits: int, salt: bytes, trailer: int = 0xBC, pad_byte: int = 0, top_bits: int = 0) -> int:
    """EMSA-PSS encoding as an integer (the signer's side, for tests): salt of any length,
    `trailer`, `pad_byte` in the first byte of PS (a corruption), `top_bits` or-ed into the
    bits of EM[0] above emBits (the BC-lenient case)."""
    em_bits = bits - 1
    em_len = (em_bits + 7) // 8
    h = hashlib.sha256(bytes(8) + hashlib.sha256(msg).digest() + salt).digest()
    db = bytearray(bytes(em_len - 33 - len(salt) - 1) + b"\x01" + salt)
    if pad_byte:
        db[1] = pad_byte
    masked = bytearray(x ^ y for x, y in zip(db, mgf1(h, len(db))))
    masked[0] &= 0xFF >> (8 * em_len - em_bits)
    masked[0] |= (top_bits << (8 - (8 * em_len - em_bits))) & 0xFF if 8 * em_len > em_bits else 0
    return int.from_bytes(bytes(masked) + h + bytes([trailer]), "big")


def sign_crt(em: int, p: int, q: int, d: int) -> int:
    """em^d mod pq by the Chinese remainder theorem."""
    sp, sq = pow(em % p, d % (p - 1), p), pow(em % q, d % (q - 1), q)
    return sq + q * (((sp - sq) * pow(q, -1, p)) % p)
