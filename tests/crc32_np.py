"""Plain-Python GF(2) restatement of the CRC-32 arithmetic (TEST INFRASTRUCTURE ONLY), for the lengths zlib
cannot be fed cheaply. A 32-bit integer holds a polynomial with the coefficient of x^0 in bit 31 (the reflected convention of
CRC-32/ISO-HDLC); P = x^32 + ... is 0xEDB88320 without its leading term."""

POLY = 0xEDB88320
ONE = 0x80000000          # x^0


def mulmod(a, b):
    """a(x) b(x) mod P"""
    p = 0
    for i in range(32):
        if (a >> (31 - i)) & 1:
            p ^= b
        b = (b >> 1) ^ (POLY if b & 1 else 0)
    return p


def xpow(e):
    """x^e mod P by square and multiply, e >= 0"""
    p, sq = ONE, ONE >> 1
    while e:
        if e & 1:
            p = mulmod(p, sq)
        sq = mulmod(sq, sq)
        e >>= 1
    return p


def raw(data, crc=0):
    """the CRC register after `data`, bit by bit, from the register value crc: no init, no final XOR"""
    for byte in data:
        crc ^= byte
        for _ in range(8):
            crc = (crc >> 1) ^ (POLY if crc & 1 else 0)
    return crc


def crc32(data):
    """zlib.crc32 restated: the init term 0xFFFFFFFF x^(8 len), the raw CRC, the final XOR"""
    return raw(data) ^ mulmod(0xFFFFFFFF, xpow(8 * len(data))) ^ 0xFFFFFFFF


def combine(crc_a, crc_b, len_b):
    """crc32(A || B) from crc32(A), crc32(B) and the length of B"""
    return mulmod(crc_a, xpow(8 * len_b)) ^ crc_b
