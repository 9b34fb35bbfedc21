"""fec_block.FECHamming / FECCyclic of scikit-dsp-comm (fec_block.py:61-423) with all four methods on the GPU (csrc/blockcode.hip).

    FECHamming(j).hamm_encoder, hamm_decoder        bit for bit the reference's outputs (float64 / int64), one launch per call
    FECCyclic(G).cyclic_encoder, cyclic_decoder     the same (int64 / int64)
    *_host                                          the same maps in vectorised NumPy over the same tables: the yardstick of the GPU tests
    hamming_tables(j), cyclic_tables(G)             the code as three tables of j-bit words

The table form.  All four methods are GF(2)-linear maps plus one compare per output bit (words are j bits wide; row 0 of H, or register
cell S[1], is the most significant bit):

    encode:  p = XOR over { i < k : x[i] = 1 } of enc[i]      code word = x[0..k) followed by bits j-1 ... 0 of p
    decode:  s = XOR over { i < n : c[i] = 1 } of syn[i]      out[i] = c[i] ^ (s == trap[i]),  i < k

Hamming: col[i] is column i of the reference's systematised H read as binary; enc = syn = col, and trap[i] is the one s in 1 ... n with
col[s - 1] - 1 == i (the reference finds the position to flip through H[:, error_pos - 1]).
Cyclic: the reference's two loops are a shift register whose zero-input step is A(S) = (S >> 1) | (parity(S & g) << (j - 1)) with g the
polynomial's digits 1 ... j.  A unit bit at position i leaves A^(count - 1 - i) applied to 1 0 ... 0 in the register, so enc[i] is the parity
read-out of A^(k - 1 - i) v0, syn[i] = A^(n - 1 - i) v0, and the decoder flips output i where A^(i + 1) s reads 1 0 ... 0, i.e. where
s == trap[i] = A^-(i + 1) v0.  A is invertible because the polynomial's last digit is 1, so every position has exactly one trap word; one
syndrome may equal several positions' trap words (non-primitive polynomials), which the per-position compare reproduces.

Deliberate differences from the reference (tests/golden/g20_conventions.json: deliberate_differences): j = 3 ... 16 only; bits must be
0 / 1 (the reference reduces anything mod 2); lists, tuples and any integer dtype are accepted; empty input returns an empty array of the
method's dtype; FECHamming.G and .R are built on first use.  ser2ber and block_single_error_Pb_bound are not part of this module.
"""
from logging import getLogger

import numpy as np

from . import _ffi

log = getLogger(__name__)

MIN_J, MAX_J = 3, 16


def _check_j(j, what):
    if int(j) != j or not MIN_J <= j <= MAX_J:
        raise ValueError("%s: j = 3 ... 16 parity bits are served (got %r)" % (what, j))
    return int(j)


# ---------------------------------------------------------------------------------------------------------------- tables
def hamming_columns(j):
    """col[i]: column i of the reference's systematised parity-check matrix read as binary (row 0 the most significant bit)"""
    j = _check_j(j, "hamming_columns")
    n = 2 ** j - 1
    col = np.arange(1, n + 1, dtype=np.int64)
    for i in range(j):                      # the reference's column swaps, in its order
        a, b = 2 ** i - 1, n - i - 1
        col[a], col[b] = col[b], col[a]
    return col


def hamming_tables(j):
    """(enc[k], syn[n], trap[k]) as uint32"""
    col = hamming_columns(j)
    n = col.size
    k = n - int(j)
    pos = np.empty(n, dtype=np.int64)       # pos[col[s - 1] - 1] = s
    pos[col - 1] = np.arange(1, n + 1)
    return col[:k].astype(np.uint32), col.astype(np.uint32), pos[:k].astype(np.uint32)


def _parity(v):
    v = v ^ (v >> 16)
    v = v ^ (v >> 8)
    v = v ^ (v >> 4)
    v = v ^ (v >> 2)
    v = v ^ (v >> 1)
    return v & 1


def _check_poly(G):
    if not isinstance(G, str) or len(G) < 2 or set(G) - {'0', '1'} or G[0] == '0' or G[-1] == '0':
        raise ValueError('Error: Invalid generator polynomial')
    _check_j(len(G) - 1, "FECCyclic")


def cyclic_tables(G):
    """(enc[k], syn[n], trap[k]) as uint32 for the generator polynomial G (a string of j + 1 binary digits, first and last '1')"""
    _check_poly(G)
    j = len(G) - 1
    n = 2 ** j - 1
    k = n - j
    g = int(G[1:], 2)                       # digit m of G (m = 1 ... j) is bit j - m: cell S[m]
    top = 1 << (j - 1)
    # v[t] = A^t v0, t < n
    v = np.empty(n, dtype=np.int64)
    s = top
    for t in range(n):
        v[t] = s
        s = (s >> 1) | ((bin(s & g).count("1") & 1) << (j - 1))
    syn = v[::-1].copy()                    # syn[i] = A^(n - 1 - i) v0
    # the parity read-out of a register: j zero-input shifts, each emitting the feedback parity, first output = most significant bit
    reg = v[:k][::-1].copy()                # the register after the message e_i: A^(k - 1 - i) v0
    enc = np.zeros(k, dtype=np.int64)
    for _ in range(j):
        enc = (enc << 1) | _parity(reg & g)
        reg >>= 1
    # trap[i] = A^-(i + 1) v0: the old cells 1 ... j - 1 are the new cells 2 ... j, the old cell j makes the feedback equal the new cell 1
    trap = np.empty(k, dtype=np.int64)
    mask = (1 << j) - 1
    u = top
    for i in range(k):
        hi = (u << 1) & mask
        u = hi | ((bin(hi & g).count("1") & 1) ^ (u >> (j - 1)))
        trap[i] = u
    return enc.astype(np.uint32), syn.astype(np.uint32), trap.astype(np.uint32)


# ---------------------------------------------------------------------------------------------------------------- the shared machinery
def _bits(x, per_block, dtype_msg, length_msg):
    """x as the kernels read it: validated, uint8 0 / 1, shape (nblocks, per_block); None for empty input"""
    x = np.asarray(x)
    if x.ndim != 1:
        raise ValueError("the bits must be a one-dimensional vector")
    if x.size == 0:
        return None
    if not np.issubdtype(x.dtype, np.integer):
        raise ValueError(dtype_msg)
    if x.size % per_block:
        raise ValueError(length_msg % per_block)
    if x.min() < 0 or x.max() > 1:
        raise ValueError("Integer bit values must be 0 or 1")
    return x.astype(np.uint8).reshape(-1, per_block)


def _word_host(bits, table):
    """per row of bits: XOR of the table words where the bit is set"""
    w = np.zeros(bits.shape[0], dtype=np.uint32)
    step = max(1, (1 << 22) // max(1, bits.shape[0]))
    for c in range(0, bits.shape[1], step):
        w ^= np.bitwise_xor.reduce(np.where(bits[:, c:c + step] != 0, table[None, c:c + step], np.uint32(0)), axis=1)
    return w


class _BlockCode(object):
    """n, k, j and the three tables; the device handle on first use"""
    _dtype_msg = 'Error: Input array should be int data type'
    _enc_len_msg = 'Error: Incomplete block in input array. Make sure input array length is a multiple of %d'
    _dec_len_msg = 'Error: Incomplete coded block in input array. Make sure coded input array length is a multiple of %d'

    def _set_tables(self, tables):
        self._enc, self._syn, self._trap = tables
        self._kern = None

    def _kernel(self):
        if self._kern is None:
            self._kern = _ffi.BlockCodeKernel(self.n, self.k, self._enc, self._syn, self._trap)
        return self._kern

    def _encode(self, x, host, out_dtype):
        b = _bits(x, self.k, self._dtype_msg, self._enc_len_msg)
        if b is None:
            return np.zeros(0, dtype=out_dtype)
        if not host:
            return self._kernel().encode(b).reshape(-1).astype(out_dtype)
        p = _word_host(b, self._enc)
        shifts = np.arange(self.j - 1, -1, -1, dtype=np.uint32)
        code = np.concatenate((b, ((p[:, None] >> shifts[None, :]) & 1).astype(np.uint8)), axis=1)
        return code.reshape(-1).astype(out_dtype)

    def _decode(self, codewords, host):
        c = _bits(codewords, self.n, self._dtype_msg, self._dec_len_msg)
        if c is None:
            return np.zeros(0, dtype=np.int64)
        if not host:
            return self._kernel().decode(c).reshape(-1).astype(np.int64)
        s = _word_host(c, self._syn)
        out = c[:, :self.k] ^ (s[:, None] == self._trap[None, :])
        return out.reshape(-1).astype(np.int64)


class FECHamming(_BlockCode):
    """(2^j - 1, 2^j - 1 - j) Hamming code: hamm_gen, hamm_encoder, hamm_decoder as in the reference."""
    _dtype_msg = 'Error: Invalid data type. Input must be a vector of ints'
    _enc_len_msg = _dec_len_msg = 'Error: Invalid input vector length. Length must be a multiple of %d'

    def __init__(self, j):
        if j < 3:
            raise ValueError('j must be > 2')
        self.j = _check_j(j, "FECHamming")
        self.n = 2 ** self.j - 1
        self.k = self.n - self.j
        col = hamming_columns(self.j)
        self.H = ((col[None, :] >> np.arange(self.j - 1, -1, -1)[:, None]) & 1).astype(int)
        self._G = self._R = None
        self._set_tables(hamming_tables(self.j))
        log.info('(%d,%d) hamming code object' % (self.n, self.k))

    @property
    def G(self):
        """Systematic generator matrix [I | P^T] (k x n), built on first use: the kernels never need it"""
        if self._G is None:
            self._G = np.zeros((self.k, self.n), dtype=int)
            self._G[:, :self.k] = np.diag(np.ones(self.k))
            self._G[:, self.k:] = self.H[:, :self.k].T
        return self._G

    @property
    def R(self):
        """[I | 0] (k x n), built on first use"""
        if self._R is None:
            self._R = np.zeros((self.k, self.n), dtype=int)
            self._R[:, :self.k] = np.diag(np.ones(self.k))
        return self._R

    def hamm_gen(self, j):
        """The reference's five values G, H, R, n, k of the order-j code (matrices of k x n integers: 133 MB each at j = 12)"""
        if j < 3:
            raise ValueError('j must be > 2')
        other = self if j == self.j else FECHamming(j)
        return other.G, other.H, other.R, other.n, other.k

    def hamm_encoder(self, x):
        """Source bits (a multiple of k) -> code words, float64 as in the reference; on the GPU"""
        return self._encode(x, False, np.float64)

    def hamm_encoder_host(self, x):
        return self._encode(x, True, np.float64)

    def hamm_decoder(self, codewords):
        """Code words (a multiple of n bits) -> corrected source bits, int64; on the GPU"""
        return self._decode(codewords, False)

    def hamm_decoder_host(self, codewords):
        return self._decode(codewords, True)


class FECCyclic(_BlockCode):
    """(2^j - 1, 2^j - 1 - j) cyclic code of the generator polynomial G (j + 1 binary digits): cyclic_encoder, cyclic_decoder."""

    def __init__(self, G='1011'):
        _check_poly(G)
        self.j = len(G) - 1
        self.n = 2 ** self.j - 1
        self.k = self.n - self.j
        self.G = G
        self._set_tables(cyclic_tables(G))
        log.info('(%d,%d) cyclic code object' % (self.n, self.k))

    def cyclic_encoder(self, x, G='1011'):
        """Source bits (a multiple of k) -> code words, int64; on the GPU.  The second argument is ignored, as in the reference."""
        return self._encode(x, False, np.int64)

    def cyclic_encoder_host(self, x, G='1011'):
        return self._encode(x, True, np.int64)

    def cyclic_decoder(self, codewords):
        """Code words (a multiple of n bits) -> decoded source bits, int64; on the GPU"""
        return self._decode(codewords, False)

    def cyclic_decoder_host(self, codewords):
        return self._decode(codewords, True)
