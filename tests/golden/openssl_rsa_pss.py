"""ctypes bridge to OpenSSL 3 libcrypto RSASSA-PSS verification (EVP_DigestVerify with
SHA-256, MGF1-SHA-256, salt length 32), an INDEPENDENT implementation used to pin
bc_rsa_pss.py, and RSA key generation / PSS signing for the golden generator."""
import ctypes
import ctypes.util

_l = None
EVP_PKEY_RSA = 6
RSA_PKCS1_PSS_PADDING = 6


def lib():
    global _l
    if _l is None:
        l = ctypes.CDLL(ctypes.util.find_library("crypto") or "libcrypto.so.3")
        vp, cp, sz, i32 = ctypes.c_void_p, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_int
        l.d2i_PublicKey.restype = vp
        l.d2i_PublicKey.argtypes = [i32, vp, ctypes.POINTER(cp), ctypes.c_long]
        l.EVP_PKEY_free.argtypes = [vp]
        l.i2d_PublicKey.argtypes = [vp, ctypes.POINTER(vp)]
        l.CRYPTO_free.argtypes = [vp, cp, i32]
        l.EVP_MD_CTX_new.restype = vp
        l.EVP_MD_CTX_free.argtypes = [vp]
        l.EVP_sha256.restype = vp
        l.EVP_DigestVerifyInit.argtypes = [vp, ctypes.POINTER(vp), vp, vp, vp]
        l.EVP_DigestVerify.argtypes = [vp, cp, sz, cp, sz]
        l.EVP_DigestSignInit.argtypes = [vp, ctypes.POINTER(vp), vp, vp, vp]
        l.EVP_DigestSign.argtypes = [vp, cp, ctypes.POINTER(sz), cp, sz]
        l.EVP_PKEY_CTX_set_rsa_padding.argtypes = [vp, i32]
        l.EVP_PKEY_CTX_set_rsa_pss_saltlen.argtypes = [vp, i32]
        l.EVP_PKEY_CTX_set_rsa_mgf1_md.argtypes = [vp, vp]
        l.EVP_PKEY_Q_keygen.restype = vp
        l.EVP_PKEY_Q_keygen.argtypes = [vp, cp, cp, sz]
        l.EVP_PKEY_get_bn_param.argtypes = [vp, cp, ctypes.POINTER(vp)]
        l.BN_num_bits.argtypes = [vp]
        l.BN_bn2bin.argtypes = [vp, cp]
        l.BN_free.argtypes = [vp]
        l.ERR_clear_error.argtypes = []
        _l = l
    return _l


def _pss(l, pctx):
    return (l.EVP_PKEY_CTX_set_rsa_padding(pctx, RSA_PKCS1_PSS_PADDING) == 1
            and l.EVP_PKEY_CTX_set_rsa_pss_saltlen(pctx, 32) == 1
            and l.EVP_PKEY_CTX_set_rsa_mgf1_md(pctx, l.EVP_sha256()) == 1)


def verify(key_der: bytes, sig: bytes, msg: bytes):
    """True / False as EVP_DigestVerify decides; None if OpenSSL rejects the key or the key
    is not the DER OpenSSL itself writes for it (key_der: DER RSAPublicKey, the SPKI BIT
    STRING payload)."""
    l = lib()
    p = ctypes.c_char_p(key_der)
    k = l.d2i_PublicKey(EVP_PKEY_RSA, None, ctypes.byref(p), len(key_der))
    if not k:
        l.ERR_clear_error()
        return None
    # d2i reads BER and stops at the end of the SEQUENCE: the key counts as accepted only if
    # OpenSSL's own DER encoding of what it read is the input, byte for byte
    out = ctypes.c_void_p()
    n = l.i2d_PublicKey(k, ctypes.byref(out))
    same = n == len(key_der) and ctypes.string_at(out, n) == key_der
    if out:
        l.CRYPTO_free(out, b"", 0)
    if not same:
        l.EVP_PKEY_free(k)
        l.ERR_clear_error()
        return None
    ctx = l.EVP_MD_CTX_new()
    try:
        pctx = ctypes.c_void_p()
        if l.EVP_DigestVerifyInit(ctx, ctypes.byref(pctx), l.EVP_sha256(), None, k) != 1 or not _pss(l, pctx):
            l.ERR_clear_error()
            return None
        r = l.EVP_DigestVerify(ctx, sig, len(sig), msg, len(msg))
        l.ERR_clear_error()
        return r == 1
    finally:
        l.EVP_MD_CTX_free(ctx)
        l.EVP_PKEY_free(k)


def _bn(l, k, name: bytes) -> int:
    bn = ctypes.c_void_p()
    assert l.EVP_PKEY_get_bn_param(k, name, ctypes.byref(bn)) == 1, name
    buf = ctypes.create_string_buffer((l.BN_num_bits(bn) + 7) // 8 or 1)
    n = l.BN_bn2bin(bn, buf)
    l.BN_free(bn)
    return int.from_bytes(buf.raw[:n], "big")


def keygen(bits: int):
    """A fresh OpenSSL RSA key (e = 65537): (handle, dict of n, e, d, p, q). Free with free_key."""
    l = lib()
    k = l.EVP_PKEY_Q_keygen(None, None, b"RSA", ctypes.c_size_t(bits))
    assert k, "EVP_PKEY_Q_keygen"
    return k, {name: _bn(l, k, param) for name, param in
               (("n", b"n"), ("e", b"e"), ("d", b"d"), ("p", b"rsa-factor1"), ("q", b"rsa-factor2"))}


def free_key(k):
    lib().EVP_PKEY_free(k)


def sign(k, msg: bytes) -> bytes:
    """RSASSA-PSS (SHA-256, MGF1-SHA-256, salt 32) signature by OpenSSL with key handle k."""
    l = lib()
    ctx = l.EVP_MD_CTX_new()
    try:
        pctx = ctypes.c_void_p()
        assert l.EVP_DigestSignInit(ctx, ctypes.byref(pctx), l.EVP_sha256(), None, k) == 1 and _pss(l, pctx)
        n = ctypes.c_size_t(0)
        assert l.EVP_DigestSign(ctx, None, ctypes.byref(n), msg, len(msg)) == 1
        buf = ctypes.create_string_buffer(n.value)
        assert l.EVP_DigestSign(ctx, buf, ctypes.byref(n), msg, len(msg)) == 1
        return buf.raw[:n.value]
    finally:
        l.EVP_MD_CTX_free(ctx)


def verify_rows(key_der: bytes, rows):
    """How many of rows [(sig, msg), ...] verify under key_der, the key parsed once and a
    fresh verification context per row: the per-signature work of a CPU verifier
    (tools/rsa_bench.py times it on several threads; ctypes drops the GIL in the calls)."""
    l = lib()
    p = ctypes.c_char_p(key_der)
    k = l.d2i_PublicKey(EVP_PKEY_RSA, None, ctypes.byref(p), len(key_der))
    assert k, "d2i_PublicKey"
    good = 0
    try:
        for sig, msg in rows:
            ctx = l.EVP_MD_CTX_new()
            pctx = ctypes.c_void_p()
            if l.EVP_DigestVerifyInit(ctx, ctypes.byref(pctx), l.EVP_sha256(), None, k) == 1 and _pss(l, pctx):
                good += l.EVP_DigestVerify(ctx, sig, len(sig), msg, len(msg)) == 1
            l.EVP_MD_CTX_free(ctx)
        l.ERR_clear_error()
    finally:
        l.EVP_PKEY_free(k)
    return good
