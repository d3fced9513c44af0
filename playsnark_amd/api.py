"""Python host mirror of the reference's Go surface for the prover hot path.

Same names, argument meaning and error behaviour as the reference, bound to the C ABI:

    Poly.BlindEval(zero, blindedPoint)   algebra.go:348-359  -> Poly.BlindEval(points)
    QAP.Quotient(sol)                    qap.go:151-162      -> QAP.Quotient(sol)
    Groth16Prove(tr, q, sol)             groth16.go:122-211  -> Groth16Prove(tr, q, sol, r, s)
    PHGR13Prove(ek, qap, solution)       pinochio.go:207-254 -> PHGR13Prove(ek, qap, solution)

The reference signals errors by panicking; here the same conditions raise
`LengthMismatch` (message of algebra.go:351) and `Apocalypse` ("apocalypse", qap.go:159).
No arithmetic happens in this file: everything is a call into libplaysnark_hip.so.
"""
from __future__ import annotations

import ctypes as C
import operator
from typing import Iterable, Optional, Sequence

from . import _lib
from ._lib import PS_G1, PS_G2, lib

G1, G2 = PS_G1, PS_G2
R_ORDER = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001  # the scalar field: encodings only, no arithmetic here
FMT_AFFINE, FMT_COMPRESSED = _lib.PS_FMT_AFFINE, _lib.PS_FMT_COMPRESSED
_WIRE = {PS_G1: 96, PS_G2: 192}


class PlaysnarkError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"playsnark_hip error {code}: {msg}")
        self.code = code


class LengthMismatch(ValueError):
    """panic(fmt.Sprintf("mismatch of length between poly %d and blinded eval points %d")) algebra.go:351"""


class Apocalypse(ArithmeticError):
    """panic("apocalypse") qap.go:159 / pinochio.go:215: the witness does not satisfy the QAP."""


def _check(rc: int):
    if rc == _lib.PS_OK:
        return
    msg = (lib.ps_last_error() or b"").decode()
    if rc == _lib.PS_ERR_LENGTH:
        raise LengthMismatch(msg)
    if rc == _lib.PS_ERR_NOT_DIVISIBLE:
        raise Apocalypse("apocalypse")
    raise PlaysnarkError(rc, msg)


def device_count() -> int:
    return lib.ps_device_count()


class Context:
    """One GPU + stream + workspace (ps_ctx)."""

    def __init__(self, device: int = 0):
        h = C.c_void_p()
        _check(lib.ps_ctx_create(device, C.byref(h)))
        self._h = h
        self.device = device

    def sync(self):
        _check(lib.ps_ctx_sync(self._h))

    @property
    def stream(self) -> int:
        return lib.ps_ctx_stream(self._h)

    def set_window(self, bits: int):
        _check(lib.ps_msm_set_window(self._h, bits))

    def set_tables(self, enable: bool):
        """Whether the provers build window tables for their CRS arrays (default: yes, for keys of >= 32 points)."""
        _check(lib.ps_ctx_set_tables(self._h, int(enable)))

    def microbench_mad(self) -> float:
        """Measured v_mad_u64_u32 issue rate in lane-operations per second (ps_microbench_mad, ~1 ms)."""
        v = C.c_double(0.0)
        _check(lib.ps_microbench_mad(self._h, C.byref(v)))
        return v.value

    def set_table_budget(self, nbytes: int):
        """Bytes a prover may spend on ONE window table (negative: automatic from the free device memory); a table that
        does not fit is skipped and the sums over that array take the plain plan."""
        _check(lib.ps_ctx_set_table_budget(self._h, nbytes))

    def set_slice(self, entries: int):
        _check(lib.ps_msm_set_slice(self._h, entries))

    def set_batch_chunk(self, members: int):
        """Members per pass of msm_batch / Groth16ProveBatch (ps_msm_batch_set_chunk); 0: automatic."""
        _check(lib.ps_msm_batch_set_chunk(self._h, members))

    def set_batch_table(self, mode: int):
        """Batched sums over the points' window tables, one bucket set per member (ps_msm_batch_set_table): 0 automatic,
        1 never (the plain pass with its fold), 2 wherever the tables are usable."""
        _check(lib.ps_msm_batch_set_table(self._h, mode))

    def set_tail(self, mode: int):
        """0 automatic, 1 chains (the long sums' tail), 2 trees of lane-cooperative additions (the short sums' tail)."""
        _check(lib.ps_msm_set_tail(self._h, mode))

    def set_accumulate(self, mode: int):
        """The point pass: 0 automatic, 1 fixed slices, 2 whole buckets in order of size (ps_msm_set_accumulate)."""
        _check(lib.ps_msm_set_accumulate(self._h, mode))

    def last_accumulate_path(self) -> int:
        """The point pass the sum finished last took: 1 slices, 2 whole buckets (0: no sum yet)."""
        path = C.c_int(0)
        _check(lib.ps_msm_last_accumulate(self._h, C.byref(path)))
        return path.value

    def prediction_counts(self) -> dict:
        """Admitted sums of this context by how their point pass was launched (ps_msm_prediction_counts): with both families,
        with the one the last sum of their kind took, and how many of the latter had to be summed again."""
        k = (C.c_uint64 * 3)()
        _check(lib.ps_msm_prediction_counts(self._h, k))
        return {"both": int(k[0]), "one": int(k[1]), "redone": int(k[2])}

    STAGES = ("digits", "scan", "scatter", "queue", "accumulate", "fixup", "reduce")

    def set_timing(self, enable: bool):
        _check(lib.ps_ctx_set_timing(self._h, int(enable)))

    def last_stage_ms(self) -> dict:
        ms = (C.c_float * len(self.STAGES))()
        _check(lib.ps_msm_last_stage_ms(self._h, ms))
        return dict(zip(self.STAGES, list(ms)))

    def last_prove_phase_ms(self) -> dict:
        """Host wall-clock split of the last Groth16Prove / PHGR13Prove on this context."""
        ms = (C.c_float * 4)()
        _check(lib.ps_prove_last_phase_ms(self._h, ms))
        return dict(zip(("quotient", "prep_or_h_sum", "sums", "total"), list(ms)))

    def last_msm_info(self) -> dict:
        info = _lib.MsmInfo()
        _check(lib.ps_msm_last_info(self._h, C.byref(info)))
        return {k: getattr(info, k) for k, _ in info._fields_}

    def close(self):
        if getattr(self, "_h", None):
            lib.ps_ctx_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Points:
    """A device-resident []G1 / []G2 slice (ps_points), e.g. Groth16Setup.Xi (groth16.go:43)."""

    def __init__(self, ctx: Context, handle, owner=None):
        self.ctx, self._h, self._owner = ctx, handle, owner

    @classmethod
    def upload(cls, ctx: Context, group: int, raw: bytes, fmt: int = _lib.PS_FMT_AFFINE) -> "Points":
        wb = _WIRE[group] if fmt == _lib.PS_FMT_AFFINE else _WIRE[group] // 2
        assert len(raw) % wb == 0
        h = C.c_void_p()
        _check(lib.ps_points_upload(ctx._h, group, raw, len(raw) // wb, fmt, C.byref(h)))
        return cls(ctx, h)

    @classmethod
    def from_scalars(cls, ctx: Context, group: int, k: "Poly") -> "Points":
        """out[i] = k[i] * G: the commit loop of GeneratePowersCommit (algebra.go:371-384)."""
        h = C.c_void_p()
        _check(lib.ps_points_from_scalars(ctx._h, group, k._h, C.byref(h)))
        return cls(ctx, h)

    @property
    def group(self) -> int:
        return lib.ps_points_group(self._h)

    def __len__(self):
        return lib.ps_points_len(self._h)

    def download(self, first: int = 0, n: Optional[int] = None) -> bytes:
        n = len(self) - first if n is None else n
        buf = C.create_string_buffer(_WIRE[self.group] * max(n, 1))
        _check(lib.ps_points_download(self.ctx._h, self._h, first, n, buf))
        return buf.raw[: _WIRE[self.group] * n]

    def download_compressed(self, first: int = 0, n: Optional[int] = None) -> bytes:
        """kyber MarshalBinary form (ZCash compressed, 48 B G1 / 96 B G2), compressed on the GPU."""
        n = len(self) - first if n is None else n
        wb = _WIRE[self.group] // 2
        buf = C.create_string_buffer(wb * max(n, 1))
        _check(lib.ps_points_download_fmt(self.ctx._h, self._h, first, n, _lib.PS_FMT_COMPRESSED, buf))
        return buf.raw[: wb * n]

    # Flat key files (the reference has no persistence): a 16-byte header
    # b"PSNK" | u8 version | u8 group | u8 format | u8 0 | u64 count (little-endian), then the points.
    def save(self, path: str, compressed: bool = True):
        import struct

        fmt = _lib.PS_FMT_COMPRESSED if compressed else _lib.PS_FMT_AFFINE
        with open(path, "wb") as f:
            f.write(b"PSNK" + struct.pack("<BBBBQ", 1, self.group, fmt, 0, len(self)))
            f.write(self.download_compressed() if compressed else self.download())

    @classmethod
    def load(cls, ctx: Context, path: str) -> "Points":
        import struct

        with open(path, "rb") as f:
            head = f.read(16)
            if len(head) != 16 or head[:4] != b"PSNK":
                raise PlaysnarkError(-3, f"{path}: not a playsnark key file")
            version, group, fmt, _, count = struct.unpack("<BBBBQ", head[4:])
            if version != 1 or group not in (PS_G1, PS_G2) or fmt not in (_lib.PS_FMT_AFFINE, _lib.PS_FMT_COMPRESSED):
                raise PlaysnarkError(-3, f"{path}: unsupported key file header")
            wb = _WIRE[group] if fmt == _lib.PS_FMT_AFFINE else _WIRE[group] // 2
            raw = f.read()
        if len(raw) != wb * count:
            raise PlaysnarkError(-1, f"{path}: {len(raw)} bytes of points, header says {count} x {wb}")
        return cls.upload(ctx, group, raw, fmt)

    def slice(self, first: int, n: int) -> "Points":
        h = C.c_void_p()
        _check(lib.ps_points_slice(self._h, first, n, C.byref(h)))
        return Points(self.ctx, h, owner=self)

    def to_lagrange(self, qap: "QAP", nodes: int = 0) -> "Points":
        """This array read as {x^i P} (a monomial-form CRS array of the reference's setups: Xi, Xi2 with nodes = 0; XiT, gsi
        with nodes = 1) -> {l_j(x) P} on the QAP's interpolation nodes (1..n, or n+1..2n-1), without the secret point
        (ps_points_monomial_to_lagrange): the one-time conversion that puts a reference-made key on the prover's fast route."""
        h = C.c_void_p()
        _check(lib.ps_points_monomial_to_lagrange(qap.ctx._h, qap._h, self._h, nodes, C.byref(h)))
        return Points(qap.ctx, h)

    def lagrange_check(self, qap: "QAP", lagr: "Points", rhos: Sequence[int], nodes: int = 0) -> bool:
        """Is `lagr` the Lagrange form of this monomial-form array, as to_lagrange(qap, nodes) makes it -- without making it
        (ps_points_lagrange_check: one interpolation over scalars and two sums)?  rhos: weights below r drawn AFTER both arrays
        are fixed, at least as many as the arrays are long (LengthMismatch otherwise, and for an array of another length than
        nbGates, or nbGates - 1 with nodes = 1)."""
        ok = C.c_int(0)
        _check(lib.ps_points_lagrange_check(qap.ctx._h, qap._h, self._h, lagr._h, nodes, _rho_bytes(rhos), len(rhos), C.byref(ok)))
        return bool(ok.value)

    def precompute(self, window_bits: int = 0) -> "Points":
        """Build the window table 2^(c w) P of this resident array once (ps_points_precompute): later sums over it,
        or over slices of it, share one bucket set.  Returns self."""
        _check(lib.ps_points_precompute(self.ctx._h, self._h, window_bits))
        return self

    def drop_table(self) -> "Points":
        """Release the window table (ps_points_precompute with window_bits = -1); sums go back to the plain plan."""
        _check(lib.ps_points_precompute(self.ctx._h, self._h, -1))
        return self

    @property
    def table_window(self) -> int:
        return lib.ps_points_table_window(self._h)

    def in_subgroup(self) -> bool:
        """[r]P = O for every point (what kyber's UnmarshalBinary enforces on the Go side [upstream])."""
        ok = C.c_int(0)
        _check(lib.ps_points_check_subgroup(self.ctx._h, self._h, C.byref(ok)))
        return bool(ok.value)

    def free(self):
        if self._h:
            lib.ps_points_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def _be32(v: int) -> bytes:
    return int(v).to_bytes(32, "big")


def _handles(polys):
    """the ps_scalars* of several Polys as one C array"""
    return (C.c_void_p * len(polys))(*[p._h.value for p in polys])


class Poly:
    """type Poly []Element (algebra.go:89), device-resident (ps_scalars).  Also stands in for
    Vector = []Value (algebra.go:13) through from_values (Value.ToFieldElement, curve.go:17-19)."""

    def __init__(self, ctx: Context, handle, owner=None):
        self.ctx, self._h, self._owner = ctx, handle, owner

    @classmethod
    def upload(cls, ctx: Context, coeffs) -> "Poly":
        raw = coeffs if isinstance(coeffs, (bytes, bytearray)) else b"".join(_be32(c) for c in coeffs)
        h = C.c_void_p()
        _check(lib.ps_scalars_upload(ctx._h, bytes(raw), len(raw) // 32, C.byref(h)))
        return cls(ctx, h)

    @classmethod
    def from_values(cls, ctx: Context, values: Sequence[int]) -> "Poly":
        arr = (C.c_int64 * len(values))(*values)
        h = C.c_void_p()
        _check(lib.ps_scalars_upload_i64(ctx._h, arr, len(values), C.byref(h)))
        return cls(ctx, h)

    @classmethod
    def from_device_be32(cls, ctx: Context, device_ptr: int, n: int) -> "Poly":
        h = C.c_void_p()
        _check(lib.ps_scalars_from_device_be32(ctx._h, C.c_void_p(device_ptr), n, C.byref(h)))
        return cls(ctx, h)

    def __len__(self):
        return lib.ps_scalars_len(self._h)

    def download_bytes(self, first: int = 0, n: Optional[int] = None) -> bytes:
        n = len(self) - first if n is None else n
        buf = C.create_string_buffer(32 * max(n, 1))
        _check(lib.ps_scalars_download(self.ctx._h, self._h, first, n, buf))
        return buf.raw[: 32 * n]

    def download(self, first: int = 0, n: Optional[int] = None):
        raw = self.download_bytes(first, n)
        return [int.from_bytes(raw[i : i + 32], "big") for i in range(0, len(raw), 32)]

    def slice(self, first: int, n: int) -> "Poly":
        h = C.c_void_p()
        _check(lib.ps_scalars_slice(self._h, first, n, C.byref(h)))
        return Poly(self.ctx, h, owner=self)

    @classmethod
    def powers(cls, ctx: Context, s: int, n: int, c: int = 1) -> "Poly":
        """[c, c s, c s^2, .., c s^(n-1)] computed on the device (ps_scalars_powers); s^0 = 1 also for s = 0.  s and c below r."""
        h = C.c_void_p()
        _check(lib.ps_scalars_powers(ctx._h, _be32(s), _be32(c), n, C.byref(h)))
        return cls(ctx, h)

    def Mul(self, p2: "Poly") -> "Poly":
        """func (p Poly) Mul(p2 Poly) Poly (algebra.go:92-105)."""
        h = C.c_void_p()
        _check(lib.ps_poly_mul(self.ctx._h, self._h, p2._h, C.byref(h)))
        return Poly(self.ctx, h)

    def BlindEval(self, blindedPoint: Points) -> bytes:
        """func (p Poly) BlindEval(zero Commit, blindedPoint []Commit) Commit (algebra.go:348).
        The group is the dynamic type of the points, as in the reference;
        `zero` is implied.  Returns the affine big-endian point (96 B G1 / 192 B G2)."""
        out = C.create_string_buffer(_WIRE[blindedPoint.group])
        _check(lib.ps_msm(self.ctx._h, blindedPoint._h, self._h, out))
        return out.raw

    def Eval(self, zs: Sequence[int]) -> list:
        """func (p Poly) Eval(i Element) Element (algebra.go:107-115) at every point of zs, on the device (ps_poly_eval)."""
        k = len(zs)
        out = C.create_string_buffer(32 * max(k, 1))
        _check(lib.ps_poly_eval(self.ctx._h, self._h, _rho_bytes(zs), k, out))
        return [int.from_bytes(out.raw[32 * j : 32 * j + 32], "big") for j in range(k)]

    def DivLinear(self, zs: Sequence[int]):
        """func (p Poly) Div(p2 Poly) (algebra.go:119-137) by the linear factors (X - z), z in zs, all at once
        (ps_poly_div_linear).  Returns (q, rems): q a Poly of len(zs) * (len(p) - 1) coefficients, row j the quotient by
        (X - zs[j]), lowest degree first -- the layout msm_batch reads -- and rems[j] = p(zs[j])."""
        k = len(zs)
        h = C.c_void_p()
        rem = C.create_string_buffer(32 * max(k, 1))
        _check(lib.ps_poly_div_linear(self.ctx._h, self._h, _rho_bytes(zs), k, C.byref(h), rem))
        return Poly(self.ctx, h), [int.from_bytes(rem.raw[32 * j : 32 * j + 32], "big") for j in range(k)]

    def DivRoots(self, zs: Sequence[int], remainder: bool = True):
        """func (p Poly) Div(p2 Poly) (algebra.go:119-137) by Z_S = prod (X - z), z in zs, len(zs) >= 1 distinct points
        (ps_poly_div_roots).  Returns (q, ys, rem): q a Poly of len(p) - len(zs) coefficients, lowest degree first (empty for
        len(p) <= len(zs)); ys[j] = p(zs[j]); rem the len(zs) coefficients of the remainder, lowest first -- the interpolant of
        (zs[j], ys[j]), made on the host in O(len(zs)^2); None with remainder=False, which skips that work."""
        k = len(zs)
        h = C.c_void_p()
        ys = C.create_string_buffer(32 * max(k, 1))
        rem = C.create_string_buffer(32 * max(k, 1)) if remainder else None
        _check(lib.ps_poly_div_roots(self.ctx._h, self._h, _rho_bytes(zs), k, C.byref(h), ys, rem))
        val = lambda buf: [int.from_bytes(buf.raw[32 * j : 32 * j + 32], "big") for j in range(k)]
        return Poly(self.ctx, h), val(ys), (val(rem) if remainder else None)

    def EvalLagrange(self, qap: "QAP", zs: Sequence[int]) -> list:
        """Eval for a polynomial held as its values on the domain 1..n of qap (self: the n values), with no interpolation
        (ps_poly_eval_lagrange).  Points may lie on the domain."""
        k = len(zs)
        out = C.create_string_buffer(32 * max(k, 1))
        _check(lib.ps_poly_eval_lagrange(self.ctx._h, qap._h, self._h, _rho_bytes(zs), k, out))
        return [int.from_bytes(out.raw[32 * j : 32 * j + 32], "big") for j in range(k)]

    def DivLinearLagrange(self, qap: "QAP", zs: Sequence[int]):
        """DivLinear for a polynomial held as its values on the domain 1..n of qap (ps_poly_div_linear_lagrange).  Returns
        (qv, ys): qv a Poly of len(zs) * n scalars, row j the VALUES on 1..n of (p - ys[j]) / (X - zs[j]) -- the layout
        msm_batch reads -- and ys[j] = p(zs[j])."""
        k = len(zs)
        h = C.c_void_p()
        ys = C.create_string_buffer(32 * max(k, 1))
        _check(lib.ps_poly_div_linear_lagrange(self.ctx._h, qap._h, self._h, _rho_bytes(zs), k, C.byref(h), ys))
        return Poly(self.ctx, h), [int.from_bytes(ys.raw[32 * j : 32 * j + 32], "big") for j in range(k)]

    def DivRootsLagrange(self, qap: "QAP", zs: Sequence[int], remainder: bool = True):
        """DivRoots for a polynomial held as its values on the domain 1..n of qap (ps_poly_div_roots_lagrange), len(zs) >= 1
        distinct points, on the domain or off it.  Returns (qv, ys, rem): qv a Poly of n scalars, the VALUES on 1..n of
        (p - r) / Z_S (all zero for len(zs) >= n); ys[j] = p(zs[j]); rem as DivRoots gives it, None with remainder=False."""
        k = len(zs)
        h = C.c_void_p()
        ys = C.create_string_buffer(32 * max(k, 1))
        rem = C.create_string_buffer(32 * max(k, 1)) if remainder else None
        _check(lib.ps_poly_div_roots_lagrange(self.ctx._h, qap._h, self._h, _rho_bytes(zs), k, C.byref(h), ys, rem))
        val = lambda buf: [int.from_bytes(buf.raw[32 * j : 32 * j + 32], "big") for j in range(k)]
        return Poly(self.ctx, h), val(ys), (val(rem) if remainder else None)

    @staticmethod
    def LinComb(polys: Sequence["Poly"], coef_matrix: Sequence[Sequence[int]]) -> "Poly":
        """len(coef_matrix[0]) rows of N = max len(p) coefficients, row j = sum_i coef_matrix[i][j] * polys[i] with every
        polynomial zero-extended to N, on the device (ps_scalars_lincomb).  One Poly of t * N coefficients, row after row -- the
        layout msm_batch and DivLinear's quotients use; slice(j * N, N) is row j.  Polynomials may be views and may repeat."""
        m = len(polys)
        if m == 0 or len(coef_matrix) != m or any(len(row) != len(coef_matrix[0]) for row in coef_matrix):
            raise LengthMismatch("Poly.LinComb: one row of coefficients per polynomial, all of one length")
        t = len(coef_matrix[0])
        ctx = polys[0].ctx
        hs = _handles(polys)
        h = C.c_void_p()
        _check(lib.ps_scalars_lincomb(ctx._h, hs, m, _rho_bytes([c for row in coef_matrix for c in row]), t, C.byref(h)))
        return Poly(ctx, h)

    def Add(self, p2: "Poly") -> "Poly":
        """func (p Poly) Add(p2 Poly) Poly (algebra.go:161-178) on the device.  The result has the length of the longer operand:
        it is NOT normalised (the reference strips leading zeros, algebra.go:230) -- finding the degree would need a pass over the
        result and a copy back, and every consumer here (sums, scans) takes zeros as they are.  Compare after normalising."""
        return Poly.LinComb([self, p2], [[1], [1]])

    def Sub(self, p2: "Poly") -> "Poly":
        """func (p Poly) Sub(p2 Poly) Poly (algebra.go:180-197) on the device; the length of the longer operand, as for Add."""
        return Poly.LinComb([self, p2], [[1], [R_ORDER - 1]])

    def free(self):
        if self._h:
            lib.ps_scalars_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def msm_launch(ctx: Context, points: Points, scalars: Poly):
    """Asynchronous BlindEval: enqueue on the context stream (ps_msm_launch)."""
    _check(lib.ps_msm_launch(ctx._h, points._h, scalars._h))


def msm_finish(ctx: Context, group: int) -> bytes:
    out = C.create_string_buffer(_WIRE[group])
    _check(lib.ps_msm_finish(ctx._h, out))
    return out.raw


def blind_eval_host(ctx: Context, points: Points, scalars) -> bytes:
    """Seam S1 as the cgo shim calls it (BlindEvalHIP -> ps_msm_be32 / ps_msm_i64): Poly.BlindEval (algebra.go:348-359) with
    the scalars still in HOST memory -- 32-byte big-endian rows as `bytes`, or a numpy int64 array of witness values
    (Value.ToFieldElement, curve.go:17-19).  The upload over PCIe is inside the call; nothing of the caller's is kept."""
    out = C.create_string_buffer(_WIRE[points.group])
    if isinstance(scalars, (bytes, bytearray)):
        _check(lib.ps_msm_be32(ctx._h, points._h, bytes(scalars), len(scalars) // 32, out))
    else:
        import numpy as np

        arr = np.ascontiguousarray(scalars, dtype=np.int64)
        _check(lib.ps_msm_i64(ctx._h, points._h, arr.ctypes.data_as(C.c_void_p), arr.size, out))
    return out.raw


def msm_multi(ctx: Context, points: list, scalars: Poly) -> list:
    """[scalars.BlindEval(p) for p in points] with one digit sort shared by all arrays (ps_msm_multi):
    the nine computeSolCommit calls of PHGR13Prove (pinochio.go:231-241) have this shape."""
    k = len(points)
    outs = [C.create_string_buffer(_WIRE[p.group]) for p in points]
    pa = (C.c_void_p * max(k, 1))(*[p._h for p in points])
    oa = (C.c_void_p * max(k, 1))(*[C.cast(o, C.c_void_p) for o in outs])
    _check(lib.ps_msm_multi(ctx._h, pa, k, scalars._h, oa))
    return [o.raw for o in outs]


def msm_batch(ctx: Context, points: Points, scalars: Poly, k: int) -> list:
    """[scalars[j*n:(j+1)*n].BlindEval(points) for j in range(k)], n = len(points), as ONE bucket problem on the device
    (ps_msm_batch): k scalar vectors back to back over one point array -- the dual of msm_multi."""
    nb = _WIRE[points.group]
    out = C.create_string_buffer(max(k, 1) * nb)
    _check(lib.ps_msm_batch(ctx._h, points._h, scalars._h, k, out))
    return [out.raw[j * nb : (j + 1) * nb] for j in range(k)]


def msm_batch_multi(ctx: Context, points: list, scalars: Poly, k: int, stride: Optional[int] = None, first: int = 0) -> list:
    """out[i][j] = scalars[j*stride + first : j*stride + first + n].BlindEval(points[i]), n = the arrays' common length
    (ps_msm_batch_multi): k scalar vectors over several point arrays, one digit sort per pass shared by all arrays and one
    bucket problem per array.  stride=None: the members back to back (stride = n).  Returns a list per array of k results."""
    a = len(points)
    if stride is None:
        stride = len(points[0]) if a else 0
    outs = [C.create_string_buffer(max(k, 1) * _WIRE[p.group]) for p in points]
    pa = (C.c_void_p * max(a, 1))(*[p._h for p in points])
    oa = (C.c_void_p * max(a, 1))(*[C.cast(o, C.c_void_p) for o in outs])
    _check(lib.ps_msm_batch_multi(ctx._h, pa, a, scalars._h, k, stride, first, oa))
    return [[o.raw[j * _WIRE[p.group] : (j + 1) * _WIRE[p.group]] for j in range(k)] for p, o in zip(points, outs)]


def point_convert(group: int, raw: bytes, in_fmt: int, out_fmt: int) -> bytes:
    """One point between the ZCash uncompressed and compressed forms (kyber MarshalBinary)."""
    out = C.create_string_buffer(_WIRE[group] if out_fmt == _lib.PS_FMT_AFFINE else _WIRE[group] // 2)
    _check(lib.ps_point_convert(group, in_fmt, out_fmt, raw, out))
    return out.raw


def points_lincomb(group: int, points: bytes, scalars: Sequence[int]) -> bytes:
    """sum_i scalars[i] * points[i] for a handful of affine points, on the host (ps_points_lincomb)."""
    out = C.create_string_buffer(_WIRE[group])
    _check(lib.ps_points_lincomb(group, points, b"".join(_be32(k % R_ORDER) for k in scalars), len(scalars), out))
    return out.raw


def msm_multi_device(ctxs: Sequence[Context], shards: Sequence[Points], scalars: Sequence["Poly"]) -> bytes:
    """One sum whose index-range shards live on several devices of this process (ps_msm_multi_device)."""
    k = len(ctxs)
    ca = (C.c_void_p * k)(*[c._h for c in ctxs])
    pa = (C.c_void_p * k)(*[p._h for p in shards])
    sa = (C.c_void_p * k)(*[s._h for s in scalars])
    out = C.create_string_buffer(_WIRE[shards[0].group])
    _check(lib.ps_msm_multi_device(ca, pa, sa, k, out))
    return out.raw


def points_sum(group: int, raw: bytes) -> bytes:
    """Sum of affine points: folds the per-GPU partial sums after the RCCL gather."""
    out = C.create_string_buffer(_WIRE[group])
    _check(lib.ps_points_sum(group, raw, len(raw) // _WIRE[group], out))
    return out.raw


# -----------------------------------------------------------------------------------------
# QAP / provers
# -----------------------------------------------------------------------------------------
_I64_MIN, _I64_MAX = -(1 << 63), (1 << 63) - 1


def _coef(v) -> int:
    """A coefficient as a Python integer; a float or any other non-integer is a TypeError (never rounded, never narrowed)."""
    if isinstance(v, int):
        return v
    try:
        return operator.index(v)
    except TypeError:
        raise TypeError("R1CS coefficients are integers, got %s" % type(v).__name__) from None


def _fits_i64(vals) -> bool:
    return all(_I64_MIN <= v <= _I64_MAX for v in vals)


def _flat(rows: Sequence[Sequence[tuple]]):
    """rows[g] = [(col, int_value), ...] -> (row_ptr, cols, vals) as Python lists; zero coefficients are dropped"""
    row_ptr = [0]
    cols, vals = [], []
    for r in rows:
        for col, v in r:
            v = _coef(v)
            if v != 0:
                cols.append(col)
                vals.append(v)
        row_ptr.append(len(cols))
    return row_ptr, cols, vals


def _pack(row_ptr, cols, vals, fr: bool):
    """(Csr or CsrFr struct, keep-alive arrays): int64 values, or 32-byte canonical big-endian values mod r"""
    a = (C.c_uint32 * len(row_ptr))(*row_ptr)
    b = (C.c_uint32 * max(len(cols), 1))(*cols)
    if fr:
        c = C.create_string_buffer(b"".join((v % R_ORDER).to_bytes(32, "big") for v in vals), max(32 * len(vals), 32))
    else:
        c = (C.c_int64 * max(len(vals), 1))(*vals)
    s = (_lib.CsrFr if fr else _lib.Csr)(C.cast(a, C.c_void_p), C.cast(b, C.c_void_p), C.cast(c, C.c_void_p))
    return s, (a, b, c)


def _csr(rows: Sequence[Sequence[tuple]], fr: Optional[bool] = None):
    """rows[g] = [(col, int_value), ...] -> (Csr struct, keep-alive arrays); a CsrFr struct of the values mod r when fr, or
    (fr = None) when some value is no int64."""
    row_ptr, cols, vals = _flat(rows)
    return _pack(row_ptr, cols, vals, (not _fits_i64(vals)) if fr is None else fr)


def _csr3(mats):
    """The three matrices for one call: int64 structs (ps_qap_create) if every coefficient of all three is an int64, else
    all three as field elements (ps_qap_create_fr).  -> (fr, structs, keep-alive)"""
    flat = [_flat(rows) for rows in mats]
    fr = not all(_fits_i64(f[2]) for f in flat)
    packed = [_pack(*f, fr) for f in flat]
    return fr, [p[0] for p in packed], [p[1] for p in packed]


def _val_is_fr(val) -> bool:
    """Is a val array of QAP.from_csr field elements (bytes, or uint8 of shape (nnz, 32)) rather than int64?"""
    mv = memoryview(val)
    if mv.format in ("e", "f", "d", "g"):
        raise TypeError("R1CS coefficients are integers, got an array of floats")
    return mv.itemsize == 1


def _csr_arrays(triples, n_gates: int):
    """QAP.from_csr's three (row_ptr, col, val) triples -> (fr, structs, keep-alive): copies of the buffers, val as int64 or
    (fr) as 32-byte field elements"""
    kinds = {_val_is_fr(val) for _, _, val in triples}
    if len(kinds) != 1:
        raise TypeError("the three val arrays must all be int64 or all be 32-byte field elements")
    fr = kinds.pop()
    structs, keep = [], []
    for row_ptr, col, val in triples:
        arrs = []
        for a, ct in ((row_ptr, C.c_uint32), (col, C.c_uint32), (val, C.c_uint8 if fr else C.c_int64)):
            raw = memoryview(a).tobytes()
            if len(raw) % C.sizeof(ct):
                raise ValueError("CSR array of the wrong element type")
            buf = (ct * max(len(raw) // C.sizeof(ct), 1))()
            C.memmove(buf, raw, len(raw))
            arrs.append((buf, len(raw) // C.sizeof(ct)))
        if arrs[0][1] != n_gates + 1:
            raise LengthMismatch("row_ptr arrays of different lengths")
        if fr and arrs[2][1] != 32 * arrs[1][1]:
            raise LengthMismatch("val holds %d bytes, 32 per column index are %d" % (arrs[2][1], 32 * arrs[1][1]))
        keep.append([a for a, _ in arrs])
        structs.append((_lib.CsrFr if fr else _lib.Csr)(*[C.cast(a, C.c_void_p) for a, _ in arrs]))
    return fr, structs, keep


def dense_to_rows(m: Sequence[Sequence[int]]):
    return [[(j, v) for j, v in enumerate(row) if v != 0] for row in m]


class QAP:
    """type QAP (qap.go:10-27), kept in the sparse evaluation form the hot path needs: the three
    R1CS matrices in CSR (rows = gates) on the reference's domain {1..n}."""

    def __init__(self, ctx: Context, nbVars: int, nbIO: int, left_rows, right_rows, out_rows):
        self.ctx = ctx
        self.nbVars, self.nbIO, self.nbGates = nbVars, nbIO, len(left_rows)
        fr, structs, keep = _csr3((left_rows, right_rows, out_rows))
        h = C.c_void_p()
        _check((lib.ps_qap_create_fr if fr else lib.ps_qap_create)(ctx._h, self.nbGates, nbVars, nbIO, C.byref(structs[0]),
                                                                   C.byref(structs[1]), C.byref(structs[2]), C.byref(h)))
        self._h = h

    @classmethod
    def from_csr(cls, ctx: Context, nbVars: int, nbIO: int, left, right, out) -> "QAP":
        """The three matrices as (row_ptr, col, val) triples of array-likes exposing the buffer protocol
        (numpy uint32 / uint32 / int64): no per-row Python lists, for circuits of millions of gates.  val may instead hold
        field elements -- an (nnz, 32) uint8 array or a bytes of 32 * nnz, canonical big-endian values -- in all three
        triples (ps_qap_create_fr); an array of floats is a TypeError."""
        self = cls.__new__(cls)
        self.ctx, self.nbVars, self.nbIO = ctx, nbVars, nbIO
        self.nbGates = len(left[0]) - 1
        fr, structs, keep = _csr_arrays((left, right, out), self.nbGates)
        h = C.c_void_p()
        _check((lib.ps_qap_create_fr if fr else lib.ps_qap_create)(ctx._h, self.nbGates, nbVars, nbIO, C.byref(structs[0]),
                                                                   C.byref(structs[1]), C.byref(structs[2]), C.byref(h)))
        self._h = h
        return self

    @classmethod
    def from_dense(cls, ctx: Context, nbVars: int, nbIO: int, left, right, out) -> "QAP":
        """ToQAP(circuit R1CS) (qap.go:35) from the dense matrices of r1cs.go:99-101."""
        return cls(ctx, nbVars, nbIO, dense_to_rows(left), dense_to_rows(right), dense_to_rows(out))

    def computeAggregatePoly(self, sol: Poly):
        """(left, right, out Poly) of qap.go:164-175 plus h in one pass."""
        hs = [C.c_void_p() for _ in range(4)]
        _check(lib.ps_qap_quotient(self.ctx._h, self._h, sol._h, *[C.byref(h) for h in hs]))
        return tuple(Poly(self.ctx, h) for h in hs)

    def interpolate(self, sol: Poly, which: int) -> Poly:
        """One of the three aggregate polynomials of computeAggregatePoly (qap.go:164-175): 0 left, 1 right, 2 out."""
        h = C.c_void_p()
        _check(lib.ps_qap_interpolate(self.ctx._h, self._h, sol._h, which, C.byref(h)))
        return Poly(self.ctx, h)

    def gate_values(self, sol: Poly, which: int) -> Poly:
        """The n values on the domain 1..n that interpolate() interpolates -- (L|R|O).sol, uninterpolated (ps_qap_gate_values):
        0 left, 1 right, 2 out.  What KZGCommitLagrange and KZGOpenLagrange take."""
        h = C.c_void_p()
        _check(lib.ps_qap_gate_values(self.ctx._h, self._h, sol._h, which, C.byref(h)))
        return Poly(self.ctx, h)

    def computeAB(self, sol: Poly):
        """(left, right, h): the Groth16 route -- A and B as coefficient vectors, h = floor(A*B / z); C is never
        interpolated (what Groth16Prove needs, groth16.go:146-185)."""
        hs = [C.c_void_p() for _ in range(3)]
        _check(lib.ps_qap_quotient(self.ctx._h, self._h, sol._h, C.byref(hs[0]), C.byref(hs[1]), None, C.byref(hs[2])))
        return tuple(Poly(self.ctx, h) for h in hs)

    def IsValid(self, sol: Poly) -> bool:
        """func (q *QAP) IsValid(sol Vector) bool (qap.go:107): does z divide left*right - out?  (A wrong number of
        solution variables panics in the reference's sanityCheck, qap.go:177-189: PlaysnarkError here.)"""
        ok = C.c_int(0)
        _check(lib.ps_qap_is_valid(self.ctx._h, self._h, sol._h, C.byref(ok)))
        return bool(ok.value)

    def Quotient(self, sol: Poly) -> Poly:
        """func (q QAP) Quotient(sol Vector) Poly (qap.go:151): raises Apocalypse when the
        remainder is non-zero."""
        h = C.c_void_p()
        _check(lib.ps_qap_quotient(self.ctx._h, self._h, sol._h, None, None, None, C.byref(h)))
        return Poly(self.ctx, h)

    def column_sums(self, which: int, points: Points) -> Points:
        """out[i] = sum_j M[j][i] * points[j] for every variable i; M = left, right, out for which = 0, 1, 2 and one point per
        gate (ps_qap_column_sums): the per-variable sums of fullLinearPoly (groth16.go:254-264) over group elements, as a
        setup without the secret point needs them.  LengthMismatch when len(points) != nbGates."""
        h = C.c_void_p()
        _check(lib.ps_qap_column_sums(self.ctx._h, self._h, which, points._h, C.byref(h)))
        return Points(self.ctx, h)

    def wide_entries(self) -> tuple:
        """(left, right, out): how many entries of each matrix have a signed magnitude min(v, r - v) of 2^64 or more
        (ps_qap_wide_entries).  (0, 0, 0) for every circuit with int64 coefficients."""
        out = (C.c_size_t * 3)()
        _check(lib.ps_qap_wide_entries(self._h, out))
        return tuple(int(v) for v in out)

    def free(self):
        if getattr(self, "_h", None):
            lib.ps_qap_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class Groth16Setup:
    """The prover's part of type Groth16Setup (groth16.go:30-61)."""

    def __init__(self, Alpha: bytes, Beta: bytes, Delta: bytes, Beta2: bytes, Delta2: bytes, Xi: Optional[Points],
                 Xi2: Optional[Points], NioLP: Points, XiT: Optional[Points], LXi: Optional[Points] = None,
                 LXi2: Optional[Points] = None, LXiT: Optional[Points] = None):
        """LXi, LXi2, LXiT: the same CRS in Lagrange form (l_j(x) G1, l_j(x) G2, lambda_k(x) t(x)/delta G1), as the device
        setup emits it; with all three the prover needs no polynomial in coefficient form (ps_groth16_pk), and Xi, Xi2, XiT
        may then be None (a Lagrange-only key: half the upload and half the device memory)."""
        lagrange = LXi is not None and LXi2 is not None and LXiT is not None
        if not lagrange and (Xi is None or Xi2 is None or XiT is None):
            raise ValueError("Groth16Setup: Xi, Xi2 and XiT may be None only when LXi, LXi2 and LXiT are all given")
        self.Alpha, self.Beta, self.Delta, self.Beta2, self.Delta2 = Alpha, Beta, Delta, Beta2, Delta2
        self.Xi, self.Xi2, self.NioLP, self.XiT = Xi, Xi2, NioLP, XiT
        self.LXi, self.LXi2, self.LXiT = LXi, LXi2, LXiT

    def monomial_only(self) -> "Groth16Setup":
        """The key as the reference's NewGroth16TrustedSetup makes it: the monomial arrays alone."""
        return Groth16Setup(self.Alpha, self.Beta, self.Delta, self.Beta2, self.Delta2, self.Xi, self.Xi2, self.NioLP, self.XiT)

    def lagrange_only(self) -> "Groth16Setup":
        """The key with its Lagrange-form arrays alone (Xi, Xi2, XiT dropped): all the fast route reads."""
        return Groth16Setup(self.Alpha, self.Beta, self.Delta, self.Beta2, self.Delta2, None, None, self.NioLP, None,
                            self.LXi, self.LXi2, self.LXiT)

    def with_lagrange(self, qap: "QAP") -> "Groth16Setup":
        """The same key with its Lagrange-form arrays computed from the monomial ones ALONE (no toxic waste, groth16.go:13-14):
        what a key made by the reference's NewGroth16TrustedSetup needs once to prove on the fast route."""
        return Groth16Setup(self.Alpha, self.Beta, self.Delta, self.Beta2, self.Delta2, self.Xi, self.Xi2, self.NioLP, self.XiT,
                            self.Xi.to_lagrange(qap, 0), self.Xi2.to_lagrange(qap, 0), self.XiT.to_lagrange(qap, 1))

    def _struct(self):
        pk = _lib.Groth16Pk()
        for name, src in (("alpha", self.Alpha), ("beta", self.Beta), ("delta", self.Delta),
                          ("beta2", self.Beta2), ("delta2", self.Delta2)):
            C.memmove(getattr(pk, name), src, len(src))
        pk.nio_lp = self.NioLP._h
        if self.Xi is not None and self.Xi2 is not None and self.XiT is not None:  # (NULL otherwise: a Lagrange-only key)
            pk.xi, pk.xi2, pk.xi_t = self.Xi._h, self.Xi2._h, self.XiT._h
        if self.LXi is not None and self.LXi2 is not None and self.LXiT is not None:
            pk.lxi, pk.lxi2, pk.lxi_t = self.LXi._h, self.LXi2._h, self.LXiT._h
        return pk


def NewGroth16TrustedSetup(qap: "QAP", alpha: int, beta: int, delta: int, x: int, gamma: int):
    """func NewGroth16TrustedSetup(qap QAP) Groth16Setup (groth16.go:64) on the device; the toxic
    waste is drawn by the caller (the reference draws it at :67-84).  Returns (Groth16Setup for the
    prover, dict with Gamma / IoLP for the verifier)."""
    tw = _lib.Groth16Toxic()
    for name, v in (("alpha", alpha), ("beta", beta), ("delta", delta), ("x", x), ("gamma", gamma)):
        C.memmove(getattr(tw, name), _be32(v), 32)
    crs = _lib.Groth16Crs()
    _check(lib.ps_groth16_setup(qap.ctx._h, qap._h, C.byref(tw), C.byref(crs)))
    pts = {f: Points(qap.ctx, C.c_void_p(getattr(crs, f))) for f in ("xi", "xi2", "io_lp", "nio_lp", "xi_t", "lxi", "lxi2", "lxi_t")}
    tr = Groth16Setup(bytes(crs.alpha), bytes(crs.beta), bytes(crs.delta), bytes(crs.beta2), bytes(crs.delta2),
                      pts["xi"], pts["xi2"], pts["nio_lp"], pts["xi_t"], pts["lxi"], pts["lxi2"], pts["lxi_t"])
    return tr, {"Gamma": bytes(crs.gamma), "IoLP": pts["io_lp"]}


class Groth16SRS:
    """Phase-1 output (a powers-of-tau string, ps_groth16_srs) for a circuit of n gates: TauG1 = {x^i G1} (2n-1 points), TauG2 =
    {x^i G2} (n), AlphaTauG1 = {alpha x^i G1} (n), BetaTauG1 = {beta x^i G1} (n), BetaG2 = beta G2 (192 bytes).  The caller
    vouches for its shape and for its points lying in the subgroup: Groth16SRSCheck tests both."""

    def __init__(self, TauG1: Points, TauG2: Points, AlphaTauG1: Points, BetaTauG1: Points, BetaG2: bytes):
        self.TauG1, self.TauG2, self.AlphaTauG1, self.BetaTauG1, self.BetaG2 = TauG1, TauG2, AlphaTauG1, BetaTauG1, BetaG2

    @classmethod
    def initial(cls, ctx: Context, m: int) -> "Groth16SRS":
        """The string a ceremony starts from, tau = alpha = beta = 1, for m gates: 2m-1, m, m, m generators."""
        ones = Poly.powers(ctx, 1, 2 * m - 1)
        g1 = Points.from_scalars(ctx, G1, ones)
        g2 = Points.from_scalars(ctx, G2, ones.slice(0, m))
        return cls(g1, g2, g1.slice(0, m), g1.slice(0, m), g2.download(0, 1))

    def truncate(self, n: int) -> "Groth16SRS":
        """Views of the first 2n-1, n, n, n points: the shape NewGroth16SetupFromSRS wants for a circuit of n gates."""
        return Groth16SRS(self.TauG1.slice(0, 2 * n - 1), self.TauG2.slice(0, n), self.AlphaTauG1.slice(0, n), self.BetaTauG1.slice(0, n),
                          self.BetaG2)

    def _struct(self):
        s = _lib.Groth16Srs()
        s.tau_g1, s.tau_g2, s.alpha_tau_g1, s.beta_tau_g1 = self.TauG1._h, self.TauG2._h, self.AlphaTauG1._h, self.BetaTauG1._h
        C.memmove(s.beta_g2, self.BetaG2, 192)
        return s


def Groth16SRSContribute(ctx: Context, srs: Groth16SRS, t: int, a: int, b: int):
    """The string with tau multiplied by t, alpha by a and beta by b (ps_groth16_srs_contribute), and the contributor's public
    share {"T2": t G2, "A2": a G2, "B2": b G2}.  t, a, b below r and non-zero; they are the caller's to draw and to delete."""
    src = srs._struct()
    out, share = _lib.Groth16Srs(), _lib.Groth16SrsShare()
    _check(lib.ps_groth16_srs_contribute(ctx._h, C.byref(src), _be32(t), _be32(a), _be32(b), C.byref(out), C.byref(share)))
    pts = [Points(ctx, C.c_void_p(getattr(out, f))) for f in ("tau_g1", "tau_g2", "alpha_tau_g1", "beta_tau_g1")]
    return Groth16SRS(*pts, bytes(out.beta_g2)), {"T2": bytes(share.t_g2), "A2": bytes(share.a_g2), "B2": bytes(share.b_g2)}


def _rho_bytes(rhos: Sequence[int]) -> bytes:
    return b"".join(int(v).to_bytes(32, "big") for v in rhos)


def Groth16SRSCheck(ctx: Context, srs: Groth16SRS, rhos: Sequence[int], check_subgroup: bool = True) -> bool:
    """Is the string well formed -- the powers of ONE tau in both groups, the same tau under alpha and beta, the same beta in G2
    (ps_groth16_srs_check)?  rhos: weights below r drawn AFTER the string is fixed, at least (longest array - 1) of them
    (LengthMismatch otherwise)."""
    s = srs._struct()
    ok = C.c_int(0)
    _check(lib.ps_groth16_srs_check(ctx._h, C.byref(s), _rho_bytes(rhos), len(rhos), int(check_subgroup), C.byref(ok)))
    return bool(ok.value)


def Groth16SRSCheckUpdate(ctx: Context, before: Groth16SRS, after: Groth16SRS, share: dict, rhos: Sequence[int]) -> bool:
    """Is `after` well formed and `before` with the (t, a, b) behind `share` folded in (ps_groth16_srs_check_update)?  `before`
    is taken as checked; that the contributor knows t, a, b is for the ceremony protocol to establish."""
    a, b = before._struct(), after._struct()
    sh = _lib.Groth16SrsShare()
    for name, key in (("t_g2", "T2"), ("a_g2", "A2"), ("b_g2", "B2")):
        C.memmove(getattr(sh, name), share[key], 192)
    ok = C.c_int(0)
    _check(lib.ps_groth16_srs_check_update(ctx._h, C.byref(a), C.byref(b), C.byref(sh), _rho_bytes(rhos), len(rhos), C.byref(ok)))
    return bool(ok.value)


def KZGCommit(tau_g1: Points, p: Poly) -> bytes:
    """func (p Poly) Commit: [p(tau)] G1 = sum_i p_i tau_g1[i] over the first len(p) powers of the string (ps_kzg_commit).
    The string may be longer than p; a shorter one raises LengthMismatch."""
    out = C.create_string_buffer(96)
    _check(lib.ps_kzg_commit(p.ctx._h, tau_g1._h, p._h, out))
    return out.raw


def KZGOpen(tau_g1: Points, p: Poly, zs: Sequence[int]):
    """(ys, proofs): ys[j] = p(zs[j]) and proofs[j] = [q_j(tau)] G1 with q_j = (p - ys[j]) / (X - zs[j]) (ps_kzg_open): values
    and quotients on the device, then one batched sum of the quotient rows over the string."""
    k = len(zs)
    ys = C.create_string_buffer(32 * max(k, 1))
    proofs = C.create_string_buffer(96 * max(k, 1))
    _check(lib.ps_kzg_open(p.ctx._h, tau_g1._h, p._h, _rho_bytes(zs), k, ys, proofs))
    return ([int.from_bytes(ys.raw[32 * j : 32 * j + 32], "big") for j in range(k)], [proofs.raw[96 * j : 96 * j + 96] for j in range(k)])


def KZGCommitLagrange(lag_g1: Points, values: Poly) -> bytes:
    """[p(tau)] G1 = sum_i v_i lag_g1[i] for a polynomial held as its values on 1..n, over the Lagrange form of the string on
    the same nodes (ps_kzg_commit_lagrange): KZGCommit's bytes for the interpolated coefficients.  Both arrays have n elements."""
    out = C.create_string_buffer(96)
    _check(lib.ps_kzg_commit_lagrange(values.ctx._h, lag_g1._h, values._h, out))
    return out.raw


def KZGOpenLagrange(qap: "QAP", lag_g1: Points, values: Poly, zs: Sequence[int]):
    """(ys, proofs) as KZGOpen gives them for the interpolated coefficients, byte for byte, from the n values on the domain of qap
    and the Lagrange form of the string (ps_kzg_open_lagrange): no interpolation and no division.  Points may lie on the domain."""
    k = len(zs)
    ys = C.create_string_buffer(32 * max(k, 1))
    proofs = C.create_string_buffer(96 * max(k, 1))
    _check(lib.ps_kzg_open_lagrange(values.ctx._h, qap._h, lag_g1._h, values._h, _rho_bytes(zs), k, ys, proofs))
    return ([int.from_bytes(ys.raw[32 * j : 32 * j + 32], "big") for j in range(k)], [proofs.raw[96 * j : 96 * j + 96] for j in range(k)])


def KZGOpenMulti(tau_g1: Points, polys: Sequence[Poly], zs: Sequence[int], coef: Sequence[Sequence[int]]):
    """(ys, proofs) for len(polys) polynomials at len(zs) points with ONE proof per point (ps_kzg_open_multi).  coef[i][j] != 0:
    polynomial i is opened at point j with this weight -- powers of a challenge drawn AFTER commitments and values are fixed.
    ys[i][j] = polys[i](zs[j]) there and None elsewhere; proofs[j] = [q_j(tau)] G1 for q_j = (f_j - f_j(z_j)) / (X - z_j),
    f_j = sum_i coef[i][j] polys[i]."""
    m, t = len(polys), len(zs)
    if len(coef) != m or any(len(row) != t for row in coef):
        raise LengthMismatch("KZGOpenMulti: coef is len(polys) rows of len(zs) weights")
    if m == 0:
        raise LengthMismatch("KZGOpenMulti: no polynomial")
    hs = _handles(polys)
    ys = C.create_string_buffer(32 * max(m * t, 1))
    proofs = C.create_string_buffer(96 * max(t, 1))
    _check(lib.ps_kzg_open_multi(polys[0].ctx._h, tau_g1._h, hs, m, _rho_bytes(zs), t, _rho_bytes([c for row in coef for c in row]), ys, proofs))
    val = lambda e: int.from_bytes(ys.raw[32 * e : 32 * e + 32], "big")
    return ([[val(i * t + j) if int(coef[i][j]) % R_ORDER else None for j in range(t)] for i in range(m)],
            [proofs.raw[96 * j : 96 * j + 96] for j in range(t)])


def KZGVerifyMulti(ctx: Context, tau_g2_1: bytes, commits: Sequence[bytes], zs: Sequence[int], coef: Sequence[Sequence[int]],
                   ys: Sequence[Sequence[Optional[int]]], proofs: Sequence[bytes], rhos: Sequence[int], check_subgroup: bool = True) -> bool:
    """What KZGOpenMulti made, in one weighted equation (ps_kzg_verify_multi): len(commits) commitments, len(zs) points, one
    proof and one non-zero weight rho per point, drawn AFTER everything else is fixed.  ys[i][j] is read where coef[i][j] != 0
    (None counts as 0 elsewhere)."""
    m, t = len(commits), len(zs)
    if not (len(proofs) == len(rhos) == t) or len(coef) != m or len(ys) != m or any(len(row) != t for row in coef) or any(len(row) != t for row in ys):
        raise LengthMismatch("KZGVerifyMulti: coef and ys are len(commits) rows of len(zs) entries; one proof and one rho per point")
    ok = C.c_int(0)
    _check(lib.ps_kzg_verify_multi(ctx._h, bytes(tau_g2_1), b"".join(commits), m, _rho_bytes(zs), t, _rho_bytes([c for row in coef for c in row]),
                                   _rho_bytes([y or 0 for row in ys for y in row]), b"".join(proofs), _rho_bytes(rhos), int(check_subgroup),
                                   C.byref(ok)))
    return bool(ok.value)


def KZGOpenSet(tau_g1: Points, p: Poly, zs: Sequence[int]):
    """(ys, proof): ys[j] = p(zs[j]) and ONE proof [q(tau)] G1 for the whole set, q = (p - r) / prod (X - zs[j]) with r the
    interpolant of the values (ps_kzg_open_set): the quotients by the single points folded into one row on the device, then
    one lone sum over the string.  len(zs) >= 1 distinct points; the identity for len(p) <= len(zs)."""
    k = len(zs)
    ys = C.create_string_buffer(32 * max(k, 1))
    proof = C.create_string_buffer(96)
    _check(lib.ps_kzg_open_set(p.ctx._h, tau_g1._h, p._h, _rho_bytes(zs), k, ys, proof))
    return [int.from_bytes(ys.raw[32 * j : 32 * j + 32], "big") for j in range(k)], proof.raw


def KZGOpenSetLagrange(qap: "QAP", lag_g1: Points, values: Poly, zs: Sequence[int]):
    """(ys, proof) as KZGOpenSet gives them for the interpolated coefficients, byte for byte, from the n values on the domain of
    qap and the Lagrange form of the string (ps_kzg_open_set_lagrange): no interpolation and no division.  len(zs) >= 1 distinct
    points, which may lie on the domain; the identity for len(zs) >= n.  KZGVerifySet checks the proof unchanged."""
    k = len(zs)
    ys = C.create_string_buffer(32 * max(k, 1))
    proof = C.create_string_buffer(96)
    _check(lib.ps_kzg_open_set_lagrange(values.ctx._h, qap._h, lag_g1._h, values._h, _rho_bytes(zs), k, ys, proof))
    return [int.from_bytes(ys.raw[32 * j : 32 * j + 32], "big") for j in range(k)], proof.raw


def KZGAllKeyLagrange(qap: "QAP", lag_g1: Points) -> Points:
    """K_m = sum_i lag_g1[i-1] / (m - i), m = 1..n (ps_kzg_all_key_lagrange): the part of the proofs of all nodes that depends on
    the domain and the string alone.  Computed once and handed to KZGOpenAllLagrange, it halves the work of every call."""
    h = C.c_void_p()
    _check(lib.ps_kzg_all_key_lagrange(qap.ctx._h, qap._h, lag_g1._h, C.byref(h)))
    return Points(qap.ctx, h)


def KZGOpenAllLagrange(qap: "QAP", lag_g1: Points, values: Poly, all_key: Optional[Points] = None) -> Points:
    """The proofs of EVERY node of the domain, proofs[m-1] = [((p - v_m) / (X - m))(tau)] G1, as n points on the device, from
    the n values on the domain of qap and the Lagrange form of the string (ps_kzg_open_all_lagrange): two transforms over points
    in place of n sums.  Each is KZGOpenLagrange's proof at z = m, byte for byte; the values at the nodes are the input itself.
    all_key: what KZGAllKeyLagrange(qap, lag_g1) returned, or None (computed inside the call and dropped)."""
    h = C.c_void_p()
    _check(lib.ps_kzg_open_all_lagrange(values.ctx._h, qap._h, lag_g1._h, all_key._h if all_key is not None else None, values._h, C.byref(h)))
    return Points(values.ctx, h)


def KZGVerifySet(ctx: Context, tau_g1: Points, tau_g2: Points, commit: bytes, zs: Sequence[int], ys: Sequence[int], proof: bytes,
                 check_subgroup: bool = True) -> bool:
    """e(C - [r(tau)] G1, G2) * e(-proof, [Z_S(tau)] G2) == 1 for what KZGOpenSet made (ps_kzg_verify_set): tau_g1 holds at least
    len(zs) powers of the string and tau_g2 at least len(zs) + 1.  A point outside the subgroup gives False (with
    check_subgroup), a malformed one raises."""
    if len(zs) != len(ys):
        raise LengthMismatch("KZGVerifySet: one value per point")
    ok = C.c_int(0)
    _check(lib.ps_kzg_verify_set(ctx._h, tau_g1._h, tau_g2._h, bytes(commit), _rho_bytes(zs), _rho_bytes(ys), len(zs), bytes(proof),
                                 int(check_subgroup), C.byref(ok)))
    return bool(ok.value)


def KZGVerify(tau_g2_1: bytes, commit: bytes, z: int, y: int, proof: bytes) -> bool:
    """e(C - y G1 + z pi, G2) == e(pi, tau G2), on the host (ps_kzg_verify); tau_g2_1 = the string's tau_g2[1].  A point outside
    the subgroup gives False, a malformed one raises."""
    ok = C.c_int(0)
    _check(lib.ps_kzg_verify(bytes(tau_g2_1), bytes(commit), _be32(z), _be32(y), bytes(proof), C.byref(ok)))
    return bool(ok.value)


def KZGVerifyBatch(ctx: Context, tau_g2_1: bytes, commits: Sequence[bytes], zs: Sequence[int], ys: Sequence[int], proofs: Sequence[bytes],
                   rhos: Sequence[int], check_subgroup: bool = True) -> bool:
    """len(commits) openings under one string in one weighted equation (ps_kzg_verify_batch).  rhos: one non-zero weight below
    r per opening, drawn AFTER everything else is fixed (128 random bits each are enough)."""
    k = len(commits)
    if not (len(zs) == len(ys) == len(proofs) == len(rhos) == k):
        raise LengthMismatch("KZGVerifyBatch: commits, zs, ys, proofs and rhos must have one length")
    ok = C.c_int(0)
    _check(lib.ps_kzg_verify_batch(ctx._h, bytes(tau_g2_1), b"".join(commits), _rho_bytes(zs), _rho_bytes(ys), b"".join(proofs), _rho_bytes(rhos), k,
                                   int(check_subgroup), C.byref(ok)))
    return bool(ok.value)


_CRS_ARRAYS =("xi", "xi2", "io_lp", "nio_lp", "xi_t", "lxi", "lxi2", "lxi_t")


def _crs_to_pair(ctx: Context, crs: "_lib.Groth16Crs"):
    """(Groth16Setup, {"Gamma", "IoLP"}) over the arrays of a filled ps_groth16_crs; the Points own the handles."""
    pts = {f: Points(ctx, C.c_void_p(getattr(crs, f))) if getattr(crs, f) else None for f in _CRS_ARRAYS}
    tr = Groth16Setup(bytes(crs.alpha), bytes(crs.beta), bytes(crs.delta), bytes(crs.beta2), bytes(crs.delta2),
                      pts["xi"], pts["xi2"], pts["nio_lp"], pts["xi_t"], pts["lxi"], pts["lxi2"], pts["lxi_t"])
    return tr, {"Gamma": bytes(crs.gamma), "IoLP": pts["io_lp"]}


def _crs_from_pair(tr: Groth16Setup, vk: dict) -> "_lib.Groth16Crs":
    crs = _lib.Groth16Crs()
    for name, src in (("alpha", tr.Alpha), ("beta", tr.Beta), ("delta", tr.Delta), ("beta2", tr.Beta2), ("delta2", tr.Delta2),
                      ("gamma", vk["Gamma"])):
        C.memmove(getattr(crs, name), src, len(src))
    for f, p in (("xi", tr.Xi), ("xi2", tr.Xi2), ("io_lp", vk["IoLP"]), ("nio_lp", tr.NioLP), ("xi_t", tr.XiT), ("lxi", tr.LXi),
                 ("lxi2", tr.LXi2), ("lxi_t", tr.LXiT)):
        if p is not None:
            setattr(crs, f, p._h)
    return crs


def NewGroth16SetupFromSRS(qap: "QAP", srs: Groth16SRS):
    """The key NewGroth16TrustedSetup(qap, alpha, beta, 1, x, 1) makes (groth16.go:64-101), byte for byte, from a powers-of-tau
    string alone: nobody's alpha, beta or x is needed (ps_groth16_setup_from_srs).  Returns the same pair, (Groth16Setup for the
    prover, dict with Gamma / IoLP for the verifier); Groth16Contribute then folds delta / gamma shares into it."""
    s = srs._struct()
    crs = _lib.Groth16Crs()
    _check(lib.ps_groth16_setup_from_srs(qap.ctx._h, qap._h, C.byref(s), C.byref(crs)))
    return _crs_to_pair(qap.ctx, crs)


def Groth16Contribute(ctx: Context, tr: Groth16Setup, vk: dict, d: int, g: int):
    """The key (tr, vk) with delta multiplied by d and gamma by g (ps_groth16_crs_contribute): NioLP, XiT, LXiT scaled by 1/d,
    IoLP by 1/g, Delta, Delta2 by d, Gamma by g.  d and g are the caller's to draw and to delete.  Returns a new pair; its Xi,
    Xi2, LXi, LXi2 share device memory with the input's (reference counted: either key may be dropped first)."""
    src = _crs_from_pair(tr, vk)
    out = _lib.Groth16Crs()
    _check(lib.ps_groth16_crs_contribute(ctx._h, C.byref(src), _be32(d % R_ORDER), _be32(g % R_ORDER), C.byref(out)))
    return _crs_to_pair(ctx, out)


def Groth16CheckUpdate(ctx: Context, before, after, rhos: Sequence[int]) -> bool:
    """Was the key `after` = (tr, vk) made from `before` = (tr, vk) by folding in SOME shares (one Groth16Contribute or several)?
    rhos: weights below r drawn AFTER both keys are fixed, at least as many as the longest of NioLP, XiT, IoLP
    (ps_groth16_crs_check_update; LengthMismatch otherwise)."""
    a, b = _crs_from_pair(*before), _crs_from_pair(*after)
    rho = b"".join(int(v).to_bytes(32, "big") for v in rhos)
    ok = C.c_int(0)
    _check(lib.ps_groth16_crs_check_update(ctx._h, C.byref(a), C.byref(b), rho, len(rhos), C.byref(ok)))
    return bool(ok.value)


def Groth16CheckFromSRS(ctx: Context, qap: "QAP", srs: Groth16SRS, key_pair, rhos: Sequence[int], check_subgroup: bool = True) -> bool:
    """Is the key `key_pair` = (tr, vk) what NewGroth16SetupFromSRS(qap, srs) makes, with SOME shares folded in (none, one
    Groth16Contribute or several) -- without deriving it again (ps_groth16_crs_check_from_srs: sums over the string with
    interpolated weights and four pairing equalities in place of five conversions over group elements)?  The Lagrange-form
    arrays are checked when the key has them.  rhos: weights below r drawn AFTER string and key are fixed, at least
    max(nbVars, nbGates) of them (LengthMismatch otherwise, and for a string of the wrong shape).  check_subgroup = False only
    for a key this process made itself."""
    s, k = srs._struct(), _crs_from_pair(*key_pair)
    ok = C.c_int(0)
    _check(lib.ps_groth16_crs_check_from_srs(ctx._h, qap._h, C.byref(s), C.byref(k), _rho_bytes(rhos), len(rhos), int(check_subgroup),
                                             C.byref(ok)))
    return bool(ok.value)


class Groth16Proof:
    """type Groth16Proof (groth16.go:106-118); tp = (R, S) as supplied."""

    def __init__(self, R, S, A, B, Cc):
        self.R, self.S, self.A, self.B, self.C = R, S, A, B, Cc


def Groth16Prove(tr: Groth16Setup, q: QAP, sol: Poly, r: int, s: int) -> Groth16Proof:
    """func Groth16Prove(tr Groth16Setup, q QAP, sol Vector) Groth16Proof (groth16.go:122).
    r and s are drawn by the caller (the reference draws them at :148 and :158)."""
    A = C.create_string_buffer(96)
    B = C.create_string_buffer(192)
    Cc = C.create_string_buffer(96)
    pk = tr._struct()
    _check(lib.ps_groth16_prove(q.ctx._h, C.byref(pk), q._h, sol._h, _be32(r), _be32(s), A, B, Cc))
    return Groth16Proof(r, s, A.raw, B.raw, Cc.raw)


def Groth16ProveBatch(tr: Groth16Setup, q: QAP, sols: Poly, rs: Sequence[int], ss: Sequence[int], valid: bool = False):
    """[Groth16Prove(tr, q, sols[j*m:(j+1)*m], rs[j], ss[j]) for j in range(len(rs))] in one call (ps_groth16_prove_batch): the
    witnesses of ONE circuit back to back in `sols`, one key, which must carry its Lagrange form (with_lagrange).
    valid=False: a list of Groth16Proof; a witness that violates a gate raises Apocalypse.  valid=True: (proofs, flags) with
    flags[j] == 0 and proof j all zero bytes for such a witness, every other proof as usual."""
    k = len(rs)
    if len(ss) != k:
        raise ValueError("Groth16ProveBatch: as many s as r")
    A, B, Cc = C.create_string_buffer(max(96 * k, 1)), C.create_string_buffer(max(192 * k, 1)), C.create_string_buffer(max(96 * k, 1))
    flags = (C.c_int * max(k, 1))() if valid else None
    pk = tr._struct()
    _check(lib.ps_groth16_prove_batch(q.ctx._h, C.byref(pk), q._h, sols._h, k, b"".join(_be32(r) for r in rs),
                                      b"".join(_be32(s) for s in ss), A, B, Cc, flags))
    proofs = [Groth16Proof(rs[j], ss[j], A.raw[96 * j : 96 * j + 96], B.raw[192 * j : 192 * j + 192], Cc.raw[96 * j : 96 * j + 96])
              for j in range(k)]
    return (proofs, list(flags)[:k]) if valid else proofs


def Groth16ProveLocal(tr_local: Groth16Setup, q: QAP, sol: Poly, r: int, s: int, rank: int, world: int):
    """One rank's share (A_part, B_part, C_part) of Groth16Prove when the rank holds ONLY its index ranges of a Lagrange-form
    key (ps_groth16_prove_local): LXi[range(n)], LXi2[range(n)], LXiT[range(n-1)], NioLP[range(nbIO)].  The element-wise
    points_sum of all ranks' parts is Groth16Prove's proof; the last rank adds the fixed points."""
    A, B, Cc = C.create_string_buffer(96), C.create_string_buffer(192), C.create_string_buffer(96)
    pk = tr_local._struct()
    _check(lib.ps_groth16_prove_local(q.ctx._h, C.byref(pk), q._h, sol._h, _be32(r), _be32(s), rank, world, A, B, Cc))
    return A.raw, B.raw, Cc.raw


def Groth16ProveMulti(devices: Sequence[tuple], r: int, s: int) -> Groth16Proof:
    """Groth16Prove over several devices of this process, each holding only its index range of the CRS arrays
    (ps_groth16_prove_multi).  devices[d] = (Groth16Setup with the d-th ranges, QAP on that device, solution on that device).
    Keys that carry LXi / LXi2 / LXiT on every device (Xi / Xi2 / XiT may be None) take the route without coefficient
    vectors; keys with the monomial arrays alone interpolate and divide."""
    arr = (_lib.Groth16Device * len(devices))()
    keep = []
    for d, (tr, q, sol) in enumerate(devices):
        pk = tr._struct()
        keep.append(pk)
        arr[d].ctx, arr[d].qap, arr[d].sol, arr[d].pk = q.ctx._h, q._h, sol._h, pk
    A, B, Cc = C.create_string_buffer(96), C.create_string_buffer(192), C.create_string_buffer(96)
    _check(lib.ps_groth16_prove_multi(arr, len(devices), _be32(r), _be32(s), A, B, Cc))
    return Groth16Proof(r, s, A.raw, B.raw, Cc.raw)


class PHGR13EvalKey:
    """type PHGR13EvalKey (pinochio.go:37-62)."""

    FIELDS = ("vs", "ws", "ys", "vas", "was", "yas", "gsi", "vbs", "wbs", "ybs")

    def __init__(self, **kw):
        for f in self.FIELDS:
            setattr(self, f, kw[f])
        self.lgsi = kw.get("lgsi")  # optional: gsi in Lagrange form on the nodes n+1..2n-1 (ps_phgr13_ek.lgsi)

    def monomial_only(self) -> "PHGR13EvalKey":
        return PHGR13EvalKey(**{f: getattr(self, f) for f in self.FIELDS})

    def with_lagrange(self, qap: "QAP") -> "PHGR13EvalKey":
        """The same key with gsi's Lagrange form on the nodes n+1..2n-1 computed from gsi alone (no toxic waste)."""
        return PHGR13EvalKey(lgsi=self.gsi.to_lagrange(qap, 1), **{f: getattr(self, f) for f in self.FIELDS})

    def _struct(self):
        ek = _lib.Phgr13Ek()
        for f in self.FIELDS:
            setattr(ek, f, getattr(self, f)._h)
        if self.lgsi is not None:
            ek.lgsi = self.lgsi._h
        return ek


class PHGR13VerifKey:
    """type PHGR13VerifKey (pinochio.go:64-91): fixed points as affine bytes, vs/ws/ys over all variables."""

    FIXED = ("av", "aw", "ay", "gamma", "bgamma", "bgamma2", "yts")

    def __init__(self, vs: Points, ws: Points, ys: Points, **fixed):
        self.vs, self.ws, self.ys = vs, ws, ys
        for f in self.FIXED:
            setattr(self, f, fixed[f])

    def fixed_points(self) -> dict:
        return {f: getattr(self, f) for f in self.FIXED}


def NewPHGR13TrustedSetup(qap: "QAP", s: int, av: int, aw: int, ay: int, rv: int, rw: int, beta: int, gamma: int):
    """func NewPHGR13TrustedSetup(qap QAP) PHGR13Setup (pinochio.go:93) on the device; the toxic waste
    is drawn by the caller, in the reference's draw order (:99-138).  Returns (EK, VK)."""
    tw = _lib.Phgr13Toxic()
    for name, v in (("s", s), ("av", av), ("aw", aw), ("ay", ay), ("rv", rv), ("rw", rw), ("beta", beta), ("gamma", gamma)):
        C.memmove(getattr(tw, name), _be32(v), 32)
    crs = _lib.Phgr13Crs()
    _check(lib.ps_phgr13_setup(qap.ctx._h, qap._h, C.byref(tw), C.byref(crs)))
    pts = {f: Points(qap.ctx, C.c_void_p(getattr(crs, f))) for f in PHGR13EvalKey.FIELDS + ("vk_vs", "vk_ws", "vk_ys", "lgsi")}
    ek = PHGR13EvalKey(lgsi=pts["lgsi"], **{f: pts[f] for f in PHGR13EvalKey.FIELDS})
    vk = PHGR13VerifKey(pts["vk_vs"], pts["vk_ws"], pts["vk_ys"], **{f: bytes(getattr(crs, f)) for f in PHGR13VerifKey.FIXED})
    return ek, vk


class PHGR13Proof:
    """type PHGR13Proof (pinochio.go:180-203)."""

    FIELDS = ("vss", "vass", "wss", "wass", "yss", "yass", "hs", "gz")

    def __init__(self, raw: _lib.Phgr13Proof):
        for f in self.FIELDS:
            setattr(self, f, bytes(getattr(raw, f)))


def PHGR13Prove(ek: PHGR13EvalKey, qap: QAP, solution: Poly) -> PHGR13Proof:
    """func PHGR13Prove(ek PHGR13EvalKey, qap QAP, solution Vector) PHGR13Proof (pinochio.go:207)."""
    out = _lib.Phgr13Proof()
    s = ek._struct()
    _check(lib.ps_phgr13_prove(qap.ctx._h, C.byref(s), qap._h, solution._h, C.byref(out)))
    return PHGR13Proof(out)


def PHGR13ProveBatch(ek: PHGR13EvalKey, qap: QAP, sols: Poly, k: int, valid: bool = False):
    """[PHGR13Prove(ek, qap, sols[j*m:(j+1)*m]) for j in range(k)] in one call (ps_phgr13_prove_batch): the witnesses of ONE
    circuit back to back in `sols`, one key, which must carry lgsi (with_lagrange; NewPHGR13TrustedSetup emits it).
    valid=False: a list of PHGR13Proof; a witness that violates a gate raises Apocalypse.  valid=True: (proofs, flags) with
    flags[j] == 0 and proof j all zero bytes for such a witness, every other proof as usual."""
    out = (_lib.Phgr13Proof * max(k, 1))()
    flags = (C.c_int * max(k, 1))() if valid else None
    s = ek._struct()
    _check(lib.ps_phgr13_prove_batch(qap.ctx._h, C.byref(s), qap._h, sols._h, k, out, flags))
    proofs = [PHGR13Proof(out[j]) for j in range(k)]
    return (proofs, list(flags)[:k]) if valid else proofs


def PHGR13ProveShard(ek: PHGR13EvalKey, qap: QAP, solution: Poly, rank: int, world: int) -> PHGR13Proof:
    """One rank's share of PHGR13Prove over the whole key (ps_phgr13_prove_shard): partial sums of the eight elements over
    the rank's index ranges.  The element-wise points_sum of all ranks' shares is PHGR13Prove's proof."""
    out = _lib.Phgr13Proof()
    s = ek._struct()
    _check(lib.ps_phgr13_prove_shard(qap.ctx._h, C.byref(s), qap._h, solution._h, rank, world, C.byref(out)))
    return PHGR13Proof(out)


def PHGR13ProveMulti(devices: Sequence[tuple]) -> PHGR13Proof:
    """PHGR13Prove over several devices of this process, each holding only its index ranges of the evaluation key
    (ps_phgr13_prove_multi).  devices[d] = (PHGR13EvalKey with the d-th ranges, QAP on that device, solution on that device)."""
    arr = (_lib.Phgr13Device * len(devices))()
    for d, (ek, q, sol) in enumerate(devices):
        arr[d].ctx, arr[d].qap, arr[d].sol, arr[d].ek = q.ctx._h, q._h, sol._h, ek._struct()
    out = _lib.Phgr13Proof()
    _check(lib.ps_phgr13_prove_multi(arr, len(devices), C.byref(out)))
    return PHGR13Proof(out)


# -----------------------------------------------------------------------------------------
# verifiers
# -----------------------------------------------------------------------------------------
def pairing_equal(a1: bytes, b1: bytes, a2: bytes, b2: bytes) -> bool:
    """Pair(a1, b1).Equal(Pair(a2, b2)) (curve.go:36-38); host-only."""
    eq = C.c_int(0)
    _check(lib.ps_pairing_equal(a1, b1, a2, b2, C.byref(eq)))
    return bool(eq.value)


def Groth16Verify(ctx: Context, Alpha: bytes, Beta2: bytes, Gamma: bytes, Delta2: bytes, IoLP: Points, p: Groth16Proof,
                  io: Poly) -> bool:
    """func Groth16Verify(tr Groth16Setup, q QAP, p Groth16Proof, io Vector) bool (groth16.go:214)."""
    vk = _lib.Groth16Vk()
    for name, src in (("alpha", Alpha), ("beta2", Beta2), ("gamma", Gamma), ("delta2", Delta2)):
        C.memmove(getattr(vk, name), src, len(src))
    vk.io_lp = IoLP._h
    ok = C.c_int(0)
    _check(lib.ps_groth16_verify(ctx._h, C.byref(vk), io._h, p.A, p.B, p.C, C.byref(ok)))
    return bool(ok.value)


def pairing_product_is_one(ctx: Context, g1: Points, g2: Points, check: bool = True) -> bool:
    """prod_i e(g1[i], g2[i]) == 1: Miller loops and their product on the device, one final exponentiation on the host.
    check=True sends both arrays through the subgroup test first (arrays from outside)."""
    one = C.c_int(0)
    _check(lib.ps_pairing_product_is_one(ctx._h, g1._h, g2._h, 1 if check else 0, C.byref(one)))
    return bool(one.value)


def Groth16VerifyBatch(ctx: Context, Alpha: bytes, Beta2: bytes, Gamma: bytes, Delta2: bytes, IoLP: Points, proofs: Sequence[Groth16Proof],
                       ios: Sequence[Poly], rhos: Sequence[int], locate: bool = False):
    """Groth16Verify (groth16.go:214) for many proofs under one key by a random linear combination with the weights `rhos`
    (non-zero, below r, drawn AFTER the proofs are fixed; 128 random bits each are enough).  ios[i] are proof i's public
    inputs (a Poly each, or ONE Poly of len(proofs) * len(IoLP) scalars, proof-major).  Returns the verdict; with locate=True
    a rejected batch is checked proof by proof with Groth16Verify and the list of the bad indices is returned instead
    (empty for an accepted batch)."""
    vk = _lib.Groth16Vk()
    for name, src in (("alpha", Alpha), ("beta2", Beta2), ("gamma", Gamma), ("delta2", Delta2)):
        C.memmove(getattr(vk, name), src, len(src))
    vk.io_lp = IoLP._h
    n, diff = len(proofs), len(IoLP)
    if isinstance(ios, Poly):
        io = ios
    else:
        if len(ios) != n:
            raise LengthMismatch(f"{len(ios)} public-input vectors for {n} proofs")
        io = Poly.upload(ctx, b"".join(v.download_bytes() for v in ios))
    raw = b"".join(bytes(p.A) + bytes(p.B) + bytes(p.C) for p in proofs)
    if len(rhos) != n:
        raise LengthMismatch(f"{len(rhos)} weights for {n} proofs")
    rho = b"".join(int(v).to_bytes(32, "big") for v in rhos)
    ok = C.c_int(0)
    _check(lib.ps_groth16_verify_batch(ctx._h, C.byref(vk), io._h, raw, n, rho, C.byref(ok)))
    if not locate:
        return bool(ok.value)
    if ok.value:
        return []
    return [i for i, p in enumerate(proofs)
            if not Groth16Verify(ctx, Alpha, Beta2, Gamma, Delta2, IoLP, p, io.slice(i * diff, diff))]


def Groth16VerifyBatchLocate(ctx: Context, Alpha: bytes, Beta2: bytes, Gamma: bytes, Delta2: bytes, IoLP: Points, proofs: Sequence[Groth16Proof],
                             ios: Sequence[Poly], rhos: Sequence[int]):
    """The invalid proofs of a batch (ps_groth16_verify_batch_locate): the batch check of Groth16VerifyBatch, then, if it
    fails, a bisection over partial results kept on the device -- at most 1 + 2 b ceil(log2 N) checks for b invalid proofs
    among N, where locate=True of Groth16VerifyBatch verifies all N one by one.  Arguments as Groth16VerifyBatch.  Returns
    (the bad indices in ascending order, info) with info = {"checks", "levels", "invalid"} of the call.  A verdict
    "invalid" is exact; "valid" is relative to the weights, like the batch verdict itself."""
    vk = _lib.Groth16Vk()
    for name, src in (("alpha", Alpha), ("beta2", Beta2), ("gamma", Gamma), ("delta2", Delta2)):
        C.memmove(getattr(vk, name), src, len(src))
    vk.io_lp = IoLP._h
    n = len(proofs)
    if isinstance(ios, Poly):
        io = ios
    else:
        if len(ios) != n:
            raise LengthMismatch(f"{len(ios)} public-input vectors for {n} proofs")
        io = Poly.upload(ctx, b"".join(v.download_bytes() for v in ios))
    raw = b"".join(bytes(p.A) + bytes(p.B) + bytes(p.C) for p in proofs)
    if len(rhos) != n:
        raise LengthMismatch(f"{len(rhos)} weights for {n} proofs")
    rho = b"".join(int(v).to_bytes(32, "big") for v in rhos)
    valid = C.create_string_buffer(max(n, 1))
    ninvalid = C.c_size_t(0)
    _check(lib.ps_groth16_verify_batch_locate(ctx._h, C.byref(vk), io._h, raw, n, rho, valid, C.byref(ninvalid)))
    raw_info = _lib.VerifyLocateInfo()
    _check(lib.ps_groth16_verify_batch_locate_info(ctx._h, C.byref(raw_info)))
    flags = valid.raw
    bad = [i for i in range(n) if flags[i] == 0]
    assert len(bad) == ninvalid.value
    return bad, {"checks": raw_info.checks, "levels": raw_info.levels, "invalid": raw_info.invalid}


def PHGR13Verify(ctx: Context, vk_points: dict, vs_io: Points, ws_io: Points, ys_io: Points, p: "PHGR13Proof", io: Poly) -> bool:
    """func PHGR13Verify(vk PHGR13VerifKey, qap QAP, p PHGR13Proof, io Vector) bool (pinochio.go:281).
    vk_points: av, aw, ay, gamma, bgamma, bgamma2, yts as affine bytes."""
    vk = _lib.Phgr13Vk()
    for name in ("av", "aw", "ay", "gamma", "bgamma", "bgamma2", "yts"):
        C.memmove(getattr(vk, name), vk_points[name], len(vk_points[name]))
    vk.vs_io, vk.ws_io, vk.ys_io = vs_io._h, ws_io._h, ys_io._h
    raw = _lib.Phgr13Proof()
    for f in PHGR13Proof.FIELDS:
        C.memmove(getattr(raw, f), getattr(p, f), len(getattr(p, f)))
    ok = C.c_int(0)
    _check(lib.ps_phgr13_verify(ctx._h, C.byref(vk), io._h, C.byref(raw), C.byref(ok)))
    return bool(ok.value)


PHGR13_EQUATIONS = ("division", "v", "w", "y", "linear")  # bit c of PHGR13VerifyBatchInfo()["failed"]: equation E_c


def _phgr13_batch_args(ctx: Context, vk_points: dict, vs_io: Points, ws_io: Points, ys_io: Points, proofs, ios, rhos):
    """(vk, io, raw proofs, n, rho bytes) as ps_phgr13_verify_batch and ps_phgr13_verify_batch_locate take them"""
    vk = _lib.Phgr13Vk()
    for name in ("av", "aw", "ay", "gamma", "bgamma", "bgamma2", "yts"):
        C.memmove(getattr(vk, name), vk_points[name], len(vk_points[name]))
    vk.vs_io, vk.ws_io, vk.ys_io = vs_io._h, ws_io._h, ys_io._h
    n = len(proofs)
    if isinstance(ios, Poly):
        io = ios
    else:
        if len(ios) != n:
            raise LengthMismatch(f"{len(ios)} public-input vectors for {n} proofs")
        io = Poly.upload(ctx, b"".join(v.download_bytes() for v in ios))
    raw = (_lib.Phgr13Proof * max(n, 1))()
    for i, p in enumerate(proofs):
        for f in PHGR13Proof.FIELDS:
            C.memmove(getattr(raw[i], f), getattr(p, f), len(getattr(p, f)))
    if len(rhos) != n:
        raise LengthMismatch(f"{len(rhos)} weights for {n} proofs")
    rho = b"".join(int(v).to_bytes(32, "big") for v in rhos)
    return vk, io, raw, n, rho


def PHGR13VerifyBatch(ctx: Context, vk_points: dict, vs_io: Points, ws_io: Points, ys_io: Points, proofs: Sequence["PHGR13Proof"],
                      ios: Sequence[Poly], rhos: Sequence[int], locate: bool = False):
    """PHGR13Verify (pinochio.go:281) for many proofs under one key (ps_phgr13_verify_batch): the five pairing products of
    the single verifier, each weighted by `rhos` (non-zero, below r, drawn AFTER the proofs are fixed; 128 random bits each
    are enough) and each checked on its own.  ios[i] are proof i's public inputs (a Poly each, or ONE Poly of
    len(proofs) * len(vs_io) scalars, proof-major).  Returns the verdict; PHGR13VerifyBatchInfo(ctx) says which of the five
    equations failed.  A malformed proof raises; there is no per-proof verdict: with locate=True a rejected batch is checked
    proof by proof with PHGR13Verify and the list of the bad indices is returned instead (empty for an accepted batch) --
    PHGR13VerifyBatchLocate finds them by bisection on the device."""
    vk, io, raw, n, rho = _phgr13_batch_args(ctx, vk_points, vs_io, ws_io, ys_io, proofs, ios, rhos)
    ok = C.c_int(0)
    _check(lib.ps_phgr13_verify_batch(ctx._h, C.byref(vk), io._h, raw, n, rho, C.byref(ok)))
    if not locate:
        return bool(ok.value)
    if ok.value:
        return []
    diff = len(vs_io)
    return [i for i, p in enumerate(proofs) if not PHGR13Verify(ctx, vk_points, vs_io, ws_io, ys_io, p, io.slice(i * diff, diff))]


def PHGR13VerifyBatchLocate(ctx: Context, vk_points: dict, vs_io: Points, ws_io: Points, ys_io: Points, proofs: Sequence["PHGR13Proof"],
                            ios: Sequence[Poly], rhos: Sequence[int]):
    """The invalid proofs of a batch and the equations each one violates (ps_phgr13_verify_batch_locate): the batch check of
    PHGR13VerifyBatch, then, if it fails, a bisection over partial results kept on the device, every half tested only on the
    equations its parent failed -- at most 1 + 2 b ceil(log2 N) checks for b invalid proofs among N, where locate=True of
    PHGR13VerifyBatch verifies all N one by one.  Arguments as PHGR13VerifyBatch.  Returns (the bad indices in ascending
    order, {index: mask of the equations that proof violates, bit c = PHGR13_EQUATIONS[c]}, info) with info = {"checks",
    "products", "levels", "invalid", "failed"} of the call.  A set bit is exact; "valid", or an unset bit, is relative to the
    weights, like the batch verdict itself."""
    vk, io, raw, n, rho = _phgr13_batch_args(ctx, vk_points, vs_io, ws_io, ys_io, proofs, ios, rhos)
    valid = C.create_string_buffer(max(n, 1))
    failed = C.create_string_buffer(max(n, 1))
    ninvalid = C.c_size_t(0)
    _check(lib.ps_phgr13_verify_batch_locate(ctx._h, C.byref(vk), io._h, raw, n, rho, valid, failed, C.byref(ninvalid)))
    raw_info = _lib.Phgr13LocateInfo()
    _check(lib.ps_phgr13_verify_batch_locate_info(ctx._h, C.byref(raw_info)))
    flags, masks = valid.raw, failed.raw
    bad = [i for i in range(n) if flags[i] == 0]
    assert len(bad) == ninvalid.value
    info = {k: getattr(raw_info, k) for k in ("checks", "products", "levels", "invalid", "failed")}
    return bad, {i: masks[i] for i in bad}, info


def PHGR13VerifyBatchInfo(ctx: Context) -> dict:
    """Of the last PHGR13VerifyBatch on ctx (ps_phgr13_verify_batch_info): {"failed": bit mask of the equations that did not
    hold (PHGR13_EQUATIONS), "device_loops": Miller loops run on the device}."""
    info = _lib.Phgr13BatchInfo()
    _check(lib.ps_phgr13_verify_batch_info(ctx._h, C.byref(info)))
    return {"failed": info.failed, "device_loops": info.device_loops}
