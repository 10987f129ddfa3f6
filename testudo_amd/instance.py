"""The public Instance / Assignment API of the reference's lib.rs:64-283: byte
encoded matrices and assignments, the padding of num_vars and num_cons, the
column shift of the (1, inputs) block, the instance digest.

    inst = Instance.new(num_cons, num_vars, num_inputs, A, B, C)   # (row, col, 32 LE bytes)
    vars_ = VarsAssignment.new([...]); inputs = InputsAssignment.new([...])
    assert inst.is_sat(ctx, vars_, inputs)

Host data only; ``to_device(ctx)`` loads the padded matrices as an
``r1cs.R1CSInstance``.  Nothing here is hot: the matrices are walked once.

``from_random_bytes`` restates the published ark-ff 0.4 rule for a prime field
with no flags: at most 32 little-endian bytes, zero-extended to 32, the top
64 * 4 - 253 = 3 bits of byte 31 cleared, None if the result is >= r.  ark-ff is
not available to check against: PARITY UNPINNED.  The reference's own
`larger_than_mod` vector (lib.rs:332-335) is rejected with or without the
masking step.
"""
from __future__ import annotations

import hashlib
import struct

import numpy as np

from .encoding import fr_array

# the scalar field modulus of BLS12-377
R = 0x12ab655e9a2ca55660b44d1e5c37b00159aa76fed00000010a11800000000001


class R1CSError(ValueError):
    """errors.rs R1CSError"""


class InvalidIndex(R1CSError):
    """a row >= num_cons or a column >= num_vars + 1 + num_inputs"""


class InvalidScalar(R1CSError):
    """bytes that are no canonical field element"""


class InvalidNumberOfInputs(R1CSError):
    """more variables than the instance has, or another number of inputs"""


def from_random_bytes(b: bytes):
    """F::from_random_bytes for Fr (ark-ff 0.4, restated; parity unpinned) -> int or None."""
    b = bytes(b)
    if len(b) > 32:
        return None
    buf = bytearray(b + bytes(32 - len(b)))
    buf[31] &= 0xFF >> 3
    v = int.from_bytes(buf, "little")
    return v if v < R else None


def scalar_bytes(v: int) -> bytes:
    """into_bigint().to_bytes_le(): the canonical value as 32 LE bytes"""
    return (v % R).to_bytes(32, "little")


def _next_pow2(n: int) -> int:
    p = 1
    while p < n:
        p *= 2
    return p


def padded_dims(num_cons: int, num_vars: int, num_inputs: int):
    """(num_cons_padded, num_vars_padded) of lib.rs:137-167 (testudo_snark.rs:48-70),
    literally: num_cons = 0 ends at 1, not 2, because 0usize.next_power_of_two()
    is 1 (lib.rs:160-162); the provers then refuse the instance (num_cons >= 2)."""
    num_vars_padded = _next_pow2(max(num_vars, num_inputs + 1))
    num_cons_padded = num_cons
    if num_cons_padded in (0, 1):
        num_cons_padded = 2
    if _next_pow2(num_cons) != num_cons:
        num_cons_padded = _next_pow2(num_cons)
    return num_cons_padded, num_vars_padded


class Assignment:
    """Assignment (lib.rs:64-113): values as integers < r"""

    def __init__(self, values):
        self.assignment = [int(v) for v in values]

    @classmethod
    def new(cls, assignment):
        """from 32-byte little-endian encodings; InvalidScalar if one does not parse"""
        vals = []
        for b in assignment:
            v = from_random_bytes(b)
            if v is None:
                raise InvalidScalar("assignment value is not a field element")
            vals.append(v)
        return cls(vals)

    def __len__(self):
        return len(self.assignment)

    def pad(self, n: int) -> "Assignment":
        assert n > len(self.assignment)
        return Assignment(self.assignment + [0] * (n - len(self.assignment)))

    def array(self) -> np.ndarray:
        """(n, 4) canonical limbs"""
        return fr_array(self.assignment) if self.assignment else np.zeros((0, 4), dtype=np.uint64)


VarsAssignment = Assignment
InputsAssignment = Assignment


class Instance:
    """Instance (lib.rs:121-283): the padded R1CSInstance and its digest."""

    def __init__(self, num_cons, num_vars, num_inputs, mats):
        self.num_cons, self.num_vars, self.num_inputs = num_cons, num_vars, num_inputs
        self.A, self.B, self.C = mats
        self.digest = self._digest()

    @classmethod
    def new(cls, num_cons, num_vars, num_inputs, A, B, C):
        """lib.rs:129-235: A, B, C lists of (row, col, value bytes)."""
        num_cons_padded, num_vars_padded = padded_dims(num_cons, num_vars, num_inputs)

        def convert(tups):
            mat = []
            for row, col, val_bytes in tups:
                if row >= num_cons:
                    raise InvalidIndex("row %d >= num_cons" % row)
                if col >= num_vars + 1 + num_inputs:
                    raise InvalidIndex("column %d >= num_vars + 1 + num_inputs" % col)
                v = from_random_bytes(val_bytes)
                if v is None:
                    raise InvalidScalar("matrix value is not a field element")
                # a column >= num_vars refers to the constant 1 or an input of the assignment
                mat.append((row, col + num_vars_padded - num_vars if col >= num_vars else col, v))
            # zero entries up to num_cons_padded when there were 0 or 1 constraints (lib.rs:199-203)
            if num_cons in (0, 1):
                for i in range(len(tups), num_cons_padded):
                    mat.append((i, num_vars, 0))
            return mat

        return cls(num_cons_padded, num_vars_padded, num_inputs, (convert(A), convert(B), convert(C)))

    @classmethod
    def from_entries(cls, num_cons, num_vars, num_inputs, A, B, C):
        """an already padded instance from (row, col, int) entries (R1CSInstance::new)"""
        if _next_pow2(num_cons) != num_cons or _next_pow2(num_vars) != num_vars or num_inputs >= num_vars:
            raise R1CSError("num_cons and num_vars must be powers of two, num_inputs < num_vars")
        return cls(num_cons, num_vars, num_inputs, tuple([(r, c, v % R) for r, c, v in M] for M in (A, B, C)))

    @property
    def num_nz_entries(self) -> int:
        return max(len(self.A), len(self.B), len(self.C), 1)

    def serialize(self) -> bytes:
        """CanonicalSerialize, Compress::Yes, of R1CSInstance { num_cons, num_vars,
        num_inputs, A, B, C } (r1csinstance.rs:20-27) with SparseMatPolynomial {
        num_vars_x, num_vars_y, M: Vec<SparseMatEntry { row, col, val }> }
        (sparse_mlpoly.rs:25-44); usize as u64 LE, entries in the order given."""
        u64 = lambda v: struct.pack("<Q", v)  # noqa: E731
        out = [u64(self.num_cons), u64(self.num_vars), u64(self.num_inputs)]
        vx, vy = self.num_cons.bit_length() - 1, (2 * self.num_vars).bit_length() - 1
        for M in (self.A, self.B, self.C):
            out += [u64(vx), u64(vy), u64(len(M))]
            out += [u64(r) + u64(c) + v.to_bytes(32, "little") for r, c, v in M]
        return b"".join(out)

    def _digest(self) -> bytes:
        """get_digest (r1csinstance.rs:155-164): 256 bytes of SHAKE-256"""
        return hashlib.shake_256(self.serialize()).digest(256)

    def _check(self, vars_: Assignment, inputs: Assignment):
        if len(vars_) > self.num_vars:
            raise InvalidNumberOfInputs("more variables than the instance has")
        if len(inputs) != self.num_inputs:
            raise InvalidNumberOfInputs("the instance has %d inputs" % self.num_inputs)

    def is_sat_host(self, vars_: Assignment, inputs: Assignment) -> bool:
        """Instance::is_sat (lib.rs:238-267) over Python integers, with padding"""
        self._check(vars_, inputs)
        z = vars_.assignment + [0] * (self.num_vars - len(vars_)) + [1] + inputs.assignment
        z += [0] * (2 * self.num_vars - len(z))
        prod = []
        for M in (self.A, self.B, self.C):
            acc = [0] * self.num_cons
            for r, c, v in M:
                acc[r] = (acc[r] + v * z[c]) % R
            prod.append(acc)
        return all(a * b % R == c for a, b, c in zip(*prod))

    def to_device(self, ctx):
        """the padded matrices as a device-resident ``r1cs.R1CSInstance``"""
        from .r1cs import R1CSInstance
        enc = lambda M: [(r, c, fr_array([v])[0]) for r, c, v in M]  # noqa: E731
        return R1CSInstance.new(ctx, self.num_cons, self.num_vars, self.num_inputs, enc(self.A), enc(self.B),
                                enc(self.C))

    def is_sat(self, ctx, vars_: Assignment, inputs: Assignment) -> bool:
        """Instance::is_sat on the device (tpst_r1cs_is_sat), the variables padded with zeros"""
        self._check(vars_, inputs)
        padded = vars_.pad(self.num_vars) if len(vars_) < self.num_vars else vars_
        return self.to_device(ctx).is_sat(padded.array(), inputs.array())


__all__ = ["Instance", "Assignment", "VarsAssignment", "InputsAssignment", "R1CSError", "InvalidIndex",
           "InvalidScalar", "InvalidNumberOfInputs", "from_random_bytes", "scalar_bytes", "padded_dims", "R"]
