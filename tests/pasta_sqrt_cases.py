"""Inputs and big-integer references shared by test_pasta_sqrt_abi.py (the host instantiation) and test_gpu_pasta_sqrt.py
(the kernels): base-field square roots on all three curves and decompression of the Pasta wire form."""
import random

from halo2_prover_amd.transcript import FIELDS, TranscriptError, compress, decompress, sqrt_mod

NOT_CANONICAL = object()          # stands for the input q + 5 in sqrt_inputs


def base_field(cid):
    return FIELDS[cid][1]


def generator(q):
    """g = z^t for the smallest non-residue z: a generator of mu_(2^32) of a Pasta base field (q - 1 = 2^32 t)"""
    t = (q - 1) >> 32
    z = 2
    while pow(z, (q - 1) // 2, q) == 1:
        z += 1
    return pow(z, t, q)


_SQRT = {}


def sqrt_inputs(cid):
    """canonical ints (and one value >= q): the edges first, then -- Pasta -- every order 2^j and every window value of the
    discrete logarithm, then 200 random elements"""
    if cid in _SQRT:
        return _SQRT[cid]
    q = base_field(cid)
    rnd = random.Random(0x5352 + cid)
    xs = [0, 1, q - 1, q + 5, 4, q - 4]
    if cid != 0:
        g = generator(q)

        def odd_part():
            return pow(rnd.randrange(1, q), 1 << 32, q)
        for j in range(33):                                    # e with exactly j trailing zero bits; j = 0: non-squares
            for _ in range(4):
                e = ((rnd.getrandbits(32) | 1) << j) & 0xFFFFFFFF
                xs.append(pow(g, e, q) * odd_part() % q)
        xs.append(odd_part())                                  # e = 0
        for w in range(4):                                     # every value of every 8-bit window of e
            for val in range(256):
                e = rnd.getrandbits(32) & ~(0xFF << (8 * w)) | (val << (8 * w))
                xs.append(pow(g, e, q) * odd_part() % q)
    xs += [rnd.randrange(q) for _ in range(200)]
    _SQRT[cid] = xs
    return xs


def is_square(a, q):
    return a % q == 0 or pow(a, (q - 1) // 2, q) == 1


def check_sqrt(cid, a, root, status):
    """the contract of h2_base_sqrt_device for one element"""
    q = base_field(cid)
    if a >= q:
        assert (root, status) == (0, 1), (hex(a), root, status)
    elif is_square(a, q):
        assert status == 0 and root < q and root * root % q == a and root % 2 == 0, (hex(a), hex(root), status)
    else:
        assert (root, status) == (0, 3), (hex(a), root, status)


_MIX = {}


def decompress_mix(cid):
    """32-byte words in the Pasta wire form: 200 points of both parities, 100 x off the curve, the edges"""
    if cid in _MIX:
        return _MIX[cid]
    q, b = base_field(cid), FIELDS[cid][2]
    rnd = random.Random(0x4D49 + cid)
    words, on, off = [], 0, 0
    while on < 200 or off < 100:
        x = rnd.randrange(q)
        y = sqrt_mod(x * x * x + b, q)
        if y is None and off < 100:
            off += 1
            words.append((x | (rnd.getrandbits(1) << 255)).to_bytes(32, "little"))
        elif y is not None and on < 200:
            words.append(compress(cid, (x, y if on % 2 else q - y)))
            on += 1
    for x in (q, q + 1, (1 << 255) - 1):
        words += [x.to_bytes(32, "little"), (x | (1 << 255)).to_bytes(32, "little")]
    words += [bytes(32), (1 << 255).to_bytes(32, "little")]   # the identity; x = 0 with the sign bit set
    rnd.shuffle(words)
    _MIX[cid] = words
    return words


def expected_point(cid, word):
    """(x, y, status) as transcript.decompress decides"""
    try:
        pt = decompress(cid, word)
    except TranscriptError as e:
        return 0, 0, 1 if "canonical" in str(e) else 3
    return (0, 0, 2) if pt is None else (pt[0], pt[1], 0)
