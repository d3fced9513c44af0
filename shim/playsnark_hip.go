// +build hip

// playsnark_hip.go -- cgo binding of libplaysnark_hip.so (include/playsnark_hip.h) for the
// nikkolasg/playsnark package.  Drop this file into the package directory and build with
// `go build -tags hip` (CGO_CFLAGS / CGO_LDFLAGS pointing at include/ and playsnark_amd/).
//
// It lives INSIDE package playsnark because the reference's key types have unexported fields
// (PHGR13EvalKey.vs .., QAP.nbVars ..).  The Go side only ever uses kyber's MarshalBinary /
// UnmarshalBinary (the reference's one serialisation site is pinochio.go:258-272): points cross the
// boundary in the ZCash compressed form those methods speak (PS_FMT_COMPRESSED on upload, batch
// decompression on the GPU; ps_point_convert on the few proof elements that come back).
//
// The image this library is built in has no Go toolchain, so this file is source only (SURVEY.md
// 8 row f4) and has never been compiled or vetted: do that first (`go vet -tags hip`) wherever Go is available.
// Every C entry point it calls -- the multi-device ones included -- is exercised by tests/abi_smoke.c (plain C) and by
// the ctypes binding the test-suite runs on.
package playsnark

/*
#cgo CFLAGS: -I${SRCDIR}/playsnark-hip/include
#cgo LDFLAGS: -L${SRCDIR}/playsnark-hip/playsnark_amd -lplaysnark_hip -Wl,-rpath,${SRCDIR}/playsnark-hip/playsnark_amd
#include <stdlib.h>
#include <string.h>
#include "playsnark_hip.h"
*/
import "C"

import (
	"fmt"
	"runtime"
	"sync"
	"unsafe"

	"github.com/drand/kyber/util/random"
)

// ---------------------------------------------------------------------------------------
// context and error mapping
// ---------------------------------------------------------------------------------------

// The reference's Groth16Prove / PHGR13Prove / BlindEval are pure functions that any number of goroutines may call.
// A ps_ctx is NOT thread-safe (one stream, one workspace, one queue of pending sums), so every use of the package
// context is serialised by hipMu.  (A pool of contexts -- one per caller, all over the same uploaded key arrays, which
// the library allows: include/playsnark_hip.h "Thread safety" -- is the way to prove from several goroutines at once.)
var (
	hipCtx *C.ps_ctx
	hipMu  sync.Mutex
)

func init() {
	if v := int(C.ps_abi_version()); v != C.PS_ABI_VERSION {
		panic(fmt.Sprintf("playsnark_hip: library ABI %d, shim written for %d", v, C.PS_ABI_VERSION))
	}
	runtime.LockOSThread() // ps_last_error is thread-local: read it on the thread that made the failing call
	defer runtime.UnlockOSThread()
	if rc := C.ps_ctx_create(0, &hipCtx); rc != C.PS_OK {
		// no CPU fallback behind this build tag: fail as loudly as the reference's own panics
		panic("playsnark_hip: " + C.GoString(C.ps_last_error()))
	}
}

// call runs one library call that uses hipCtx: under the context's lock, and pinned to its OS thread so that
// ps_last_error() (thread-local in the library) is read on the thread the failing call ran on -- a goroutine may
// otherwise be rescheduled onto another thread between two cgo calls.  Error codes map onto the reference's panics.
func call(f func() C.int) {
	hipMu.Lock()
	runtime.LockOSThread()
	rc := f()
	msg := ""
	if rc != C.PS_OK {
		msg = C.GoString(C.ps_last_error())
	}
	runtime.UnlockOSThread()
	hipMu.Unlock()
	switch rc {
	case C.PS_OK:
	case C.PS_ERR_NOT_DIVISIBLE:
		panic("apocalypse") // qap.go:159, pinochio.go:215
	default:
		// PS_ERR_LENGTH carries the message of algebra.go:351, PS_ERR_ARG that of sanityCheck (qap.go:177-189)
		panic(msg)
	}
}

// check is `call` for the entry points that touch no context (ps_point_convert, ps_points_sum, ..).
func check(f func() C.int) {
	runtime.LockOSThread()
	rc := f()
	msg := ""
	if rc != C.PS_OK {
		msg = C.GoString(C.ps_last_error())
	}
	runtime.UnlockOSThread()
	if rc != C.PS_OK {
		panic(msg)
	}
}

func u8(b []byte) *C.uint8_t {
	if len(b) == 0 {
		return nil
	}
	return (*C.uint8_t)(unsafe.Pointer(&b[0]))
}

// ---------------------------------------------------------------------------------------
// byte forms: only MarshalBinary / UnmarshalBinary on the Go side
// ---------------------------------------------------------------------------------------

const (
	g1Wire = 96 // PS_FMT_AFFINE sizes; MarshalBinary emits half of these (compressed)
	g2Wire = 192
)

func wireLen(group C.int) int {
	if group == C.PS_G1 {
		return g1Wire
	}
	return g2Wire
}

func marshalPoints(pts []Commit) []byte {
	out := make([]byte, 0, len(pts)*g2Wire/2)
	for _, p := range pts {
		b, err := p.MarshalBinary() // 48 B (G1) / 96 B (G2), ZCash compressed
		if err != nil {
			panic(err)
		}
		out = append(out, b...)
	}
	return out
}

func marshalScalars(p Poly) []byte {
	out := make([]byte, 0, 32*len(p))
	for _, e := range p {
		b, err := e.MarshalBinary() // 32-byte big-endian (kyber mod.Int)
		if err != nil {
			panic(err)
		}
		out = append(out, b...)
	}
	return out
}

// affineOf gives the uncompressed bytes the fixed-point fields of the C structs take.
func affineOf(group C.int, p Commit) []byte {
	in, err := p.MarshalBinary()
	if err != nil {
		panic(err)
	}
	out := make([]byte, wireLen(group))
	check(func() C.int { return C.ps_point_convert(group, C.PS_FMT_COMPRESSED, C.PS_FMT_AFFINE, u8(in), u8(out)) })
	return out
}

// pointFrom turns an affine result of the library back into a kyber point of the group of `like`.
func pointFrom(group C.int, affine []byte, like Commit) Commit {
	comp := make([]byte, wireLen(group)/2)
	check(func() C.int { return C.ps_point_convert(group, C.PS_FMT_AFFINE, C.PS_FMT_COMPRESSED, u8(affine), u8(comp)) })
	p := like.Clone()
	if err := p.UnmarshalBinary(comp); err != nil {
		panic(err)
	}
	return p
}

func copyTo(dst unsafe.Pointer, src []byte) {
	C.memcpy(dst, unsafe.Pointer(&src[0]), C.size_t(len(src)))
}

// uploadPoints keeps a CRS slice resident in HBM (once per setup, reused by every proof).  The byte
// slice is not retained by the library past the call (cgo pointer rules).
func uploadPoints(group C.int, pts []Commit) *C.ps_points {
	raw := marshalPoints(pts)
	var h *C.ps_points
	call(func() C.int { return C.ps_points_upload(hipCtx, group, u8(raw), C.size_t(len(pts)), C.PS_FMT_COMPRESSED, &h) })
	return h
}

// uploadSolution: Vector = []Value = []int (algebra.go:13); Value.ToFieldElement is SetInt64 (curve.go:17-19).
func uploadSolution(sol Vector) *C.ps_scalars {
	vals := make([]C.int64_t, len(sol))
	for i, v := range sol {
		vals[i] = C.int64_t(v)
	}
	var h *C.ps_scalars
	var p *C.int64_t
	if len(vals) > 0 {
		p = &vals[0]
	}
	call(func() C.int { return C.ps_scalars_upload_i64(hipCtx, p, C.size_t(len(vals)), &h) })
	return h
}

func downloadPoly(h *C.ps_scalars) Poly {
	n := int(C.ps_scalars_len(h))
	raw := make([]byte, 32*n)
	call(func() C.int { return C.ps_scalars_download(hipCtx, h, 0, C.size_t(n), u8(raw)) })
	out := make(Poly, n)
	for i := range out {
		e := NewElement()
		if err := e.UnmarshalBinary(raw[32*i : 32*i+32]); err != nil {
			panic(err)
		}
		out[i] = e
	}
	return out
}

// ---------------------------------------------------------------------------------------
// Poly.BlindEval (algebra.go:348-359) and Poly.Mul (algebra.go:92-105)
// ---------------------------------------------------------------------------------------

func groupOf(zero Commit) C.int {
	// the group is the DYNAMIC type of the points (declared Go types lie: Xi2 []G1 at groth16.go:60)
	if len(mustMarshal(zero)) == g1Wire/2 {
		return C.PS_G1
	}
	return C.PS_G2
}

func mustMarshal(p Commit) []byte {
	b, err := p.MarshalBinary()
	if err != nil {
		panic(err)
	}
	return b
}

// BlindEvalHIP replaces `func (p Poly) BlindEval(zero Commit, blindedPoint []Commit) Commit` for a
// CRS slice that was uploaded once with uploadPoints.
func (p Poly) BlindEvalHIP(zero Commit, crs *C.ps_points) Commit {
	if int(C.ps_points_len(crs)) != len(p) { // the reference's own panic and message, algebra.go:350-352
		panic(fmt.Sprintf("mismatch of length between poly %d and blinded eval points %d", len(p), int(C.ps_points_len(crs))))
	}
	group := C.ps_points_group(crs)
	sc := marshalScalars(p)
	out := make([]byte, wireLen(group))
	call(func() C.int { return C.ps_msm_be32(hipCtx, crs, u8(sc), C.size_t(len(p)), u8(out)) })
	return pointFrom(group, out, zero)
}

// MulHIP replaces `func (p Poly) Mul(p2 Poly) Poly`.
func (p Poly) MulHIP(p2 Poly) Poly {
	var a, b, prod *C.ps_scalars
	ra, rb := marshalScalars(p), marshalScalars(p2)
	call(func() C.int { return C.ps_scalars_upload(hipCtx, u8(ra), C.size_t(len(p)), &a) })
	defer C.ps_scalars_free(a)
	call(func() C.int { return C.ps_scalars_upload(hipCtx, u8(rb), C.size_t(len(p2)), &b) })
	defer C.ps_scalars_free(b)
	call(func() C.int { return C.ps_poly_mul(hipCtx, a, b, &prod) })
	defer C.ps_scalars_free(prod)
	return downloadPoly(prod)
}

// ---------------------------------------------------------------------------------------
// QAP: the R1CS matrices (r1cs.go:78-101, rows = gates, columns = variables) in CSR.  The arrays a
// ps_csr points at must not be Go memory holding Go pointers, so they are staged in C memory.
// ---------------------------------------------------------------------------------------

type cCsr struct {
	csr         C.ps_csr
	rp, col, va unsafe.Pointer
}

func newCsr(m Matrix) *cCsr {
	nnz := 0
	for _, row := range m {
		for _, v := range row {
			if v != 0 {
				nnz++
			}
		}
	}
	c := &cCsr{
		rp:  C.malloc(C.size_t(4 * (len(m) + 1))),
		col: C.malloc(C.size_t(4*nnz + 4)),
		va:  C.malloc(C.size_t(8*nnz + 8)),
	}
	rp := (*[1 << 30]C.uint32_t)(c.rp)[: len(m)+1 : len(m)+1]
	col := (*[1 << 30]C.uint32_t)(c.col)[: nnz+1 : nnz+1]
	va := (*[1 << 29]C.int64_t)(c.va)[: nnz+1 : nnz+1]
	k := 0
	for g, row := range m {
		rp[g] = C.uint32_t(k)
		for j, v := range row {
			if v != 0 {
				col[k] = C.uint32_t(j)
				va[k] = C.int64_t(v)
				k++
			}
		}
	}
	rp[len(m)] = C.uint32_t(k)
	c.csr.row_ptr = (*C.uint32_t)(c.rp)
	c.csr.col = (*C.uint32_t)(c.col)
	c.csr.val = (*C.int64_t)(c.va)
	return c
}

func (c *cCsr) free() {
	C.free(c.rp)
	C.free(c.col)
	C.free(c.va)
}

// HipQAP is the device-resident counterpart of ToQAP(circuit) (qap.go:35-65): the per-variable
// polynomials are never materialised, the quotient works from the sparse matrices on the domain {1..n}.
type HipQAP struct {
	h                     *C.ps_qap
	nbVars, nbIO, nbGates int
}

func NewHipQAP(circuit R1CS) *HipQAP {
	l, r, o := newCsr(circuit.left), newCsr(circuit.right), newCsr(circuit.out)
	defer l.free()
	defer r.free()
	defer o.free()
	q := &HipQAP{nbVars: len(circuit.vars), nbIO: circuit.nbIO(), nbGates: len(circuit.left)}
	call(func() C.int { return C.ps_qap_create(hipCtx, C.size_t(q.nbGates), C.size_t(q.nbVars), C.size_t(q.nbIO), &l.csr, &r.csr, &o.csr, &q.h) })
	return q
}

// FrCsr is one R1CS matrix (rows = gates) whose coefficients are field elements: Val[k] is the canonical 32-byte big-endian
// value of entry k (the format of kyber's Scalar.MarshalBinary).  The reference's Value is an int (algebra.go:11); a front end
// that emits round constants, MDS entries or weights 2^k for k >= 64 needs this form.
type FrCsr struct {
	RowPtr []uint32 // nbGates + 1
	Col    []uint32 // nnz
	Val    [][32]byte
}

type cCsrFr struct {
	csr         C.ps_csr_fr
	rp, col, va unsafe.Pointer
}

func newCsrFr(m FrCsr) *cCsrFr {
	nnz := len(m.Col)
	if len(m.Val) != nnz {
		panic(fmt.Sprintf("FrCsr: %d column indices and %d values", nnz, len(m.Val)))
	}
	c := &cCsrFr{
		rp:  C.malloc(C.size_t(4 * len(m.RowPtr))),
		col: C.malloc(C.size_t(4*nnz + 4)),
		va:  C.malloc(C.size_t(32*nnz + 32)),
	}
	rp := (*[1 << 30]C.uint32_t)(c.rp)[:len(m.RowPtr):len(m.RowPtr)]
	col := (*[1 << 30]C.uint32_t)(c.col)[: nnz+1 : nnz+1]
	va := (*[1 << 30]byte)(c.va)[: 32*nnz+32 : 32*nnz+32]
	for g, v := range m.RowPtr {
		rp[g] = C.uint32_t(v)
	}
	for k := 0; k < nnz; k++ {
		col[k] = C.uint32_t(m.Col[k])
		copy(va[32*k:32*k+32], m.Val[k][:])
	}
	c.csr.row_ptr = (*C.uint32_t)(c.rp)
	c.csr.col = (*C.uint32_t)(c.col)
	c.csr.val_be32 = (*C.uint8_t)(c.va)
	return c
}

func (c *cCsrFr) free() {
	C.free(c.rp)
	C.free(c.col)
	C.free(c.va)
}

// NewHipQAPFr is NewHipQAP for matrices with field coefficients (ps_qap_create_fr).  A coefficient not below r panics
// (PS_ERR_ENCODING), as does a column index out of range.
func NewHipQAPFr(nbVars, nbIO int, left, right, out FrCsr) *HipQAP {
	if len(left.RowPtr) == 0 || len(right.RowPtr) != len(left.RowPtr) || len(out.RowPtr) != len(left.RowPtr) {
		panic("NewHipQAPFr: the three matrices need the same, non-zero number of gates")
	}
	l, r, o := newCsrFr(left), newCsrFr(right), newCsrFr(out)
	defer l.free()
	defer r.free()
	defer o.free()
	q := &HipQAP{nbVars: nbVars, nbIO: nbIO, nbGates: len(left.RowPtr) - 1}
	call(func() C.int { return C.ps_qap_create_fr(hipCtx, C.size_t(q.nbGates), C.size_t(q.nbVars), C.size_t(q.nbIO), &l.csr, &r.csr, &o.csr, &q.h) })
	return q
}

// WideEntries: how many entries of left, right and out have a signed magnitude min(v, r - v) of 2^64 or more
// (ps_qap_wide_entries); 0, 0, 0 for every circuit made by NewHipQAP.
func (q *HipQAP) WideEntries() [3]int {
	var w [3]C.size_t
	call(func() C.int { return C.ps_qap_wide_entries(q.h, &w[0]) })
	return [3]int{int(w[0]), int(w[1]), int(w[2])}
}

func (q *HipQAP) Free() { C.ps_qap_free(q.h) }

// QuotientHIP replaces `func (q QAP) Quotient(sol Vector) Poly` (qap.go:151-162): panics "apocalypse"
// when the witness does not satisfy the circuit.
func (q *HipQAP) QuotientHIP(sol Vector) Poly {
	dsol := uploadSolution(sol)
	defer C.ps_scalars_free(dsol)
	var h *C.ps_scalars
	call(func() C.int { return C.ps_qap_quotient(hipCtx, q.h, dsol, nil, nil, nil, &h) })
	defer C.ps_scalars_free(h)
	return downloadPoly(h)
}

// IsValidHIP replaces `func (q *QAP) IsValid(sol Vector) bool` (qap.go:107-148): does z(x) divide
// left(x) right(x) - out(x)?  On the device: the three SpMVs and the gate check of the quotient.
func (q *HipQAP) IsValidHIP(sol Vector) bool {
	dsol := uploadSolution(sol)
	defer C.ps_scalars_free(dsol)
	var ok C.int
	call(func() C.int { return C.ps_qap_is_valid(hipCtx, q.h, dsol, &ok) })
	return ok != 0
}

// ---------------------------------------------------------------------------------------
// Groth16 (groth16.go)
// ---------------------------------------------------------------------------------------

// HipGroth16 holds what Groth16Prove / Groth16Verify need on the device: the CRS arrays of a
// Groth16Setup uploaded once, and the QAP.
type HipGroth16 struct {
	pk                        C.ps_groth16_pk
	vk                        C.ps_groth16_vk
	xi, xi2, nioLP, xiT, ioLP *C.ps_points
	lagrange                  []*C.ps_points // lxi, lxi2, lxi_t when the key came from NewHipGroth16FromToxicWaste
	crs                       C.ps_groth16_crs // the whole key when it came from NewHipGroth16FromSRS / ContributeHIP
	qap                       *HipQAP
}

func NewHipGroth16(tr Groth16Setup, q *HipQAP) *HipGroth16 {
	hs := &HipGroth16{qap: q}
	hs.xi = uploadPoints(C.PS_G1, tr.Xi)
	hs.xi2 = uploadPoints(C.PS_G2, tr.Xi2) // declared []G1 at groth16.go:60, holds G2 points
	hs.nioLP = uploadPoints(C.PS_G1, tr.NioLP)
	hs.xiT = uploadPoints(C.PS_G1, tr.XiT)
	hs.ioLP = uploadPoints(C.PS_G1, tr.IoLP)
	copyTo(unsafe.Pointer(&hs.pk.alpha[0]), affineOf(C.PS_G1, tr.Alpha))
	copyTo(unsafe.Pointer(&hs.pk.beta[0]), affineOf(C.PS_G1, tr.Beta))
	copyTo(unsafe.Pointer(&hs.pk.delta[0]), affineOf(C.PS_G1, tr.Delta))
	copyTo(unsafe.Pointer(&hs.pk.beta2[0]), affineOf(C.PS_G2, tr.Beta2))
	copyTo(unsafe.Pointer(&hs.pk.delta2[0]), affineOf(C.PS_G2, tr.Delta2))
	hs.pk.xi, hs.pk.xi2, hs.pk.nio_lp, hs.pk.xi_t = hs.xi, hs.xi2, hs.nioLP, hs.xiT
	copyTo(unsafe.Pointer(&hs.vk.alpha[0]), affineOf(C.PS_G1, tr.Alpha))
	copyTo(unsafe.Pointer(&hs.vk.beta2[0]), affineOf(C.PS_G2, tr.Beta2))
	copyTo(unsafe.Pointer(&hs.vk.gamma[0]), affineOf(C.PS_G2, tr.Gamma))
	copyTo(unsafe.Pointer(&hs.vk.delta2[0]), affineOf(C.PS_G2, tr.Delta2))
	hs.vk.io_lp = hs.ioLP
	return hs
}

// ToLagrange puts a key made by the reference's NewGroth16TrustedSetup (monomial arrays only) onto the prover's fast route
// WITHOUT the toxic waste, which "must be delete[d] after a trusted setup" (groth16.go:13-14): Xi, Xi2 and XiT are converted
// on the GPU into l_j(x) G1, l_j(x) G2 and lambda_k(x) t(x)/delta G1 over the group elements alone
// (ps_points_monomial_to_lagrange: a transposed interpolation, seconds at 2^16 gates, under a minute at 2^20 -- once per key).
// Afterwards Groth16ProveHIP needs no interpolation and no division; the proof bytes do not change.
func (hs *HipGroth16) ToLagrange() {
	if hs.pk.lxi != nil {
		return
	}
	var lxi, lxi2, lxit *C.ps_points
	call(func() C.int { return C.ps_points_monomial_to_lagrange(hipCtx, hs.qap.h, hs.xi, 0, &lxi) })
	call(func() C.int { return C.ps_points_monomial_to_lagrange(hipCtx, hs.qap.h, hs.xi2, 0, &lxi2) })
	call(func() C.int { return C.ps_points_monomial_to_lagrange(hipCtx, hs.qap.h, hs.xiT, 1, &lxit) })
	hs.lagrange = []*C.ps_points{lxi, lxi2, lxit}
	hs.pk.lxi, hs.pk.lxi2, hs.pk.lxi_t = lxi, lxi2, lxit
}

// NewHipGroth16FromToxicWaste builds the device-resident key from the five scalars the reference's setup keeps
// "for testing and learning purpose" (groth16.go:13-27, tr.tw): ps_groth16_setup recomputes every CRS array on the
// GPU -- the same points, byte for byte, as tr.Xi, tr.Xi2, tr.IoLP, tr.NioLP, tr.XiT -- and emits the SAME CRS in
// Lagrange form beside them (ps_groth16_pk.lxi / lxi2 / lxi_t), with which the prover needs no interpolation and no
// division (a 2^20-constraint proof in 21.5 ms instead of 32.5).  Nothing is uploaded through MarshalBinary.
func NewHipGroth16FromToxicWaste(tr Groth16Setup, q *HipQAP) *HipGroth16 {
	var tw C.ps_groth16_toxic
	put := func(dst *C.uint8_t, e Element) {
		b, err := e.MarshalBinary()
		if err != nil {
			panic(err)
		}
		copyTo(unsafe.Pointer(dst), b)
	}
	put(&tw.alpha[0], tr.tw.Alpha)
	put(&tw.beta[0], tr.tw.Beta)
	put(&tw.delta[0], tr.tw.Delta)
	put(&tw.x[0], tr.tw.X)
	put(&tw.gamma[0], tr.tw.Gamma)
	var crs C.ps_groth16_crs
	call(func() C.int { return C.ps_groth16_setup(hipCtx, q.h, &tw, &crs) })
	hs := &HipGroth16{qap: q, xi: crs.xi, xi2: crs.xi2, nioLP: crs.nio_lp, xiT: crs.xi_t, ioLP: crs.io_lp}
	hs.lagrange = []*C.ps_points{crs.lxi, crs.lxi2, crs.lxi_t}
	hs.pk.alpha, hs.pk.beta, hs.pk.delta, hs.pk.beta2, hs.pk.delta2 = crs.alpha, crs.beta, crs.delta, crs.beta2, crs.delta2
	hs.pk.xi, hs.pk.xi2, hs.pk.nio_lp, hs.pk.xi_t = crs.xi, crs.xi2, crs.nio_lp, crs.xi_t
	hs.pk.lxi, hs.pk.lxi2, hs.pk.lxi_t = crs.lxi, crs.lxi2, crs.lxi_t
	hs.vk.alpha, hs.vk.beta2, hs.vk.gamma, hs.vk.delta2 = crs.alpha, crs.beta2, crs.gamma, crs.delta2
	hs.vk.io_lp = crs.io_lp
	return hs
}

func (hs *HipGroth16) Free() {
	for _, p := range append([]*C.ps_points{hs.xi, hs.xi2, hs.nioLP, hs.xiT, hs.ioLP}, hs.lagrange...) {
		C.ps_points_free(p)
	}
}

// Groth16ProveHIP replaces `func Groth16Prove(tr Groth16Setup, q QAP, sol Vector) Groth16Proof`
// (groth16.go:122-211).  r and s are drawn exactly as the reference draws them (:148, :158) and
// handed to the library, which is deterministic.
func Groth16ProveHIP(hs *HipGroth16, sol Vector) Groth16Proof {
	r := NewElement().Pick(random.New())
	s := NewElement().Pick(random.New())
	rb, _ := r.MarshalBinary()
	sb, _ := s.MarshalBinary()
	dsol := uploadSolution(sol)
	defer C.ps_scalars_free(dsol)
	A := make([]byte, g1Wire)
	B := make([]byte, g2Wire)
	Cc := make([]byte, g1Wire)
	call(func() C.int { return C.ps_groth16_prove(hipCtx, &hs.pk, hs.qap.h, dsol, u8(rb), u8(sb), u8(A), u8(B), u8(Cc)) })
	return Groth16Proof{
		tp: groth16ToxicProof{R: r, S: s},
		A:  pointFrom(C.PS_G1, A, zeroG1),
		B:  pointFrom(C.PS_G2, B, zeroG2),
		C:  pointFrom(C.PS_G1, Cc, zeroG1),
	}
}

// Groth16ProveBatchHIP is Groth16ProveHIP for many witnesses of ONE circuit under one key, in one call
// (ps_groth16_prove_batch): one pass of wire values and gate checks over all witnesses, then three batched sums.  The
// route is the Lagrange-form one, so a key that came from the reference's setup is converted first (ToLagrange, once per
// key).  Proof j is the proof Groth16ProveHIP would make of sols[j] with the same (r, s), which are drawn here per proof.
// A witness that violates a gate panics with the reference's "apocalypse" (qap.go:158-160).
func Groth16ProveBatchHIP(hs *HipGroth16, sols []Vector) []Groth16Proof {
	k := len(sols)
	if k == 0 {
		return nil
	}
	hs.ToLagrange()
	flat := make(Vector, 0, k*len(sols[0]))
	for _, s := range sols {
		if len(s) != len(sols[0]) {
			panic("Groth16ProveBatchHIP: the witnesses of one circuit have one length")
		}
		flat = append(flat, s...)
	}
	rs, ss := make([]Element, k), make([]Element, k)
	rb, sb := make([]byte, 0, 32*k), make([]byte, 0, 32*k)
	for j := 0; j < k; j++ {
		rs[j] = NewElement().Pick(random.New())
		ss[j] = NewElement().Pick(random.New())
		b, _ := rs[j].MarshalBinary()
		rb = append(rb, b...)
		b, _ = ss[j].MarshalBinary()
		sb = append(sb, b...)
	}
	dsols := uploadSolution(flat)
	defer C.ps_scalars_free(dsols)
	A := make([]byte, g1Wire*k)
	B := make([]byte, g2Wire*k)
	Cc := make([]byte, g1Wire*k)
	call(func() C.int {
		return C.ps_groth16_prove_batch(hipCtx, &hs.pk, hs.qap.h, dsols, C.size_t(k), u8(rb), u8(sb), u8(A), u8(B), u8(Cc), nil)
	})
	out := make([]Groth16Proof, k)
	for j := range out {
		out[j] = Groth16Proof{
			tp: groth16ToxicProof{R: rs[j], S: ss[j]},
			A:  pointFrom(C.PS_G1, A[g1Wire*j:g1Wire*(j+1)], zeroG1),
			B:  pointFrom(C.PS_G2, B[g2Wire*j:g2Wire*(j+1)], zeroG2),
			C:  pointFrom(C.PS_G1, Cc[g1Wire*j:g1Wire*(j+1)], zeroG1),
		}
	}
	return out
}

// SetBatchTableHIP says whether the batched sums (BlindEvalBatchHIP, the batch provers) run over the window tables of their
// points, one bucket set per member (ps_msm_batch_set_table): 0 automatic, 1 never, 2 wherever the tables are usable.
func SetBatchTableHIP(mode int) {
	call(func() C.int { return C.ps_msm_batch_set_table(hipCtx, C.int(mode)) })
}

// BlindEvalBatchHIP is BlindEvalHIP for k polynomials over ONE array of blinded points, as one bucket problem on the
// device (ps_msm_batch): out[j] = polys[j].BlindEval(zero, crs).
func BlindEvalBatchHIP(polys []Poly, zero Commit, crs *C.ps_points) []Commit {
	k := len(polys)
	n := int(C.ps_points_len(crs))
	sc := make([]byte, 0, 32*k*n)
	for _, p := range polys {
		if len(p) != n { // the reference's own panic and message, algebra.go:350-352
			panic(fmt.Sprintf("mismatch of length between poly %d and blinded eval points %d", len(p), n))
		}
		sc = append(sc, marshalScalars(p)...)
	}
	group := C.ps_points_group(crs)
	var h *C.ps_scalars
	call(func() C.int { return C.ps_scalars_upload(hipCtx, u8(sc), C.size_t(k*n), &h) })
	defer C.ps_scalars_free(h)
	w := wireLen(group)
	raw := make([]byte, w*k)
	call(func() C.int { return C.ps_msm_batch(hipCtx, crs, h, C.size_t(k), u8(raw)) })
	out := make([]Commit, k)
	for j := range out {
		out[j] = pointFrom(group, raw[w*j:w*(j+1)], zero)
	}
	return out
}

// Groth16VerifyHIP replaces `func Groth16Verify(tr Groth16Setup, q QAP, p Groth16Proof, io Vector) bool`
// (groth16.go:214-233): pairings on the host inside the library, the IO sum on the GPU.  A proof point
// that is not a canonical encoding of a subgroup element never gets here: UnmarshalBinary refused it.
func Groth16VerifyHIP(hs *HipGroth16, p Groth16Proof, io Vector) bool {
	dio := uploadSolution(io)
	defer C.ps_scalars_free(dio)
	var ok C.int
	call(func() C.int { return C.ps_groth16_verify(hipCtx, &hs.vk, dio, u8(affineOf(C.PS_G1, p.A)), u8(affineOf(C.PS_G2, p.B)),
		u8(affineOf(C.PS_G1, p.C)), &ok) })
	return ok != 0
}

// Groth16VerifyBatchHIP checks many proofs under one key with ONE final exponentiation (ps_groth16_verify_batch): the
// weights of the random linear combination are drawn here, after the proofs are in hand, 128 bits each.
func Groth16VerifyBatchHIP(hs *HipGroth16, proofs []Groth16Proof, ios []Vector) bool {
	if len(proofs) != len(ios) {
		panic("Groth16VerifyBatchHIP: one public-input vector per proof")
	}
	if len(proofs) == 0 {
		return true
	}
	var all Vector
	raw := make([]byte, 0, 384*len(proofs))
	rho := make([]byte, 32*len(proofs))
	for i, p := range proofs {
		all = append(all, ios[i]...)
		raw = append(raw, affineOf(C.PS_G1, p.A)...)
		raw = append(raw, affineOf(C.PS_G2, p.B)...)
		raw = append(raw, affineOf(C.PS_G1, p.C)...)
		for zero := true; zero; { // 128 random bits, drawn again in the (2^-128) case that they are all zero
			random.Bytes(rho[32*i+16:32*i+32], random.New())
			for _, b := range rho[32*i+16 : 32*i+32] {
				zero = zero && b == 0
			}
		}
	}
	dio := uploadSolution(all)
	defer C.ps_scalars_free(dio)
	var ok C.int
	call(func() C.int {
		return C.ps_groth16_verify_batch(hipCtx, &hs.vk, dio, u8(raw), C.size_t(len(proofs)), u8(rho), &ok)
	})
	return ok != 0
}

// Groth16VerifyBatchLocateHIP names the invalid proofs of a batch (ps_groth16_verify_batch_locate): the batch check of
// Groth16VerifyBatchHIP first, then, if it fails, a bisection over partial results kept on the device -- at most
// 1 + 2 b ceil(log2 N) checks for b invalid proofs among N.  The weights are drawn here, as in Groth16VerifyBatchHIP.
// Returns the indices of the invalid proofs in ascending order (nil for an accepted batch) and the number of checks.
func Groth16VerifyBatchLocateHIP(hs *HipGroth16, proofs []Groth16Proof, ios []Vector) ([]int, int) {
	if len(proofs) != len(ios) {
		panic("Groth16VerifyBatchLocateHIP: one public-input vector per proof")
	}
	if len(proofs) == 0 {
		return nil, 0
	}
	var all Vector
	raw := make([]byte, 0, 384*len(proofs))
	rho := make([]byte, 32*len(proofs))
	for i, p := range proofs {
		all = append(all, ios[i]...)
		raw = append(raw, affineOf(C.PS_G1, p.A)...)
		raw = append(raw, affineOf(C.PS_G2, p.B)...)
		raw = append(raw, affineOf(C.PS_G1, p.C)...)
		for zero := true; zero; {
			random.Bytes(rho[32*i+16:32*i+32], random.New())
			for _, b := range rho[32*i+16 : 32*i+32] {
				zero = zero && b == 0
			}
		}
	}
	dio := uploadSolution(all)
	defer C.ps_scalars_free(dio)
	valid := make([]byte, len(proofs))
	var ninvalid C.size_t
	var info C.ps_verify_locate_info
	call(func() C.int {
		return C.ps_groth16_verify_batch_locate(hipCtx, &hs.vk, dio, u8(raw), C.size_t(len(proofs)), u8(rho), u8(valid), &ninvalid)
	})
	call(func() C.int { return C.ps_groth16_verify_batch_locate_info(hipCtx, &info) })
	var bad []int
	for i, v := range valid {
		if v == 0 {
			bad = append(bad, i)
		}
	}
	return bad, int(info.checks)
}

// ---------------------------------------------------------------------------------------
// A key from a powers-of-tau string: NewGroth16TrustedSetup (groth16.go:64-101) keeps alpha, beta, delta, x, gamma "for
// testing and learning purpose" (groth16.go:13-14).  A deployment derives the circuit's key from a universal string
// {x^i G} nobody knows (delta = gamma = 1), every party folds a delta / gamma share of its own into it, and anybody checks
// a fold.
// ---------------------------------------------------------------------------------------

// ColumnSumsHIP: out[i] = sum_j M[j][i] * pts[j] over the variables i, M = left, right, out for which = 0, 1, 2
// (ps_qap_column_sums): fullLinearPoly's per-variable sums (groth16.go:254-264) over group elements.  The caller frees.
func (q *HipQAP) ColumnSumsHIP(which int, pts *C.ps_points) *C.ps_points {
	var out *C.ps_points
	call(func() C.int { return C.ps_qap_column_sums(hipCtx, q.h, C.int(which), pts, &out) })
	return out
}

// Groth16SRS is phase-1 output for a circuit of n gates: TauG1 = {x^i G1} (2n-1), TauG2 = {x^i G2} (n), AlphaTauG1 =
// {alpha x^i G1} (n), BetaTauG1 = {beta x^i G1} (n), BetaG2 = beta G2.  UnmarshalBinary has put every point in the subgroup.
type Groth16SRS struct {
	TauG1, TauG2, AlphaTauG1, BetaTauG1 []Commit
	BetaG2                              Commit
}

// hipGroth16FromCrs wraps a whole ps_groth16_crs: both forms of the arrays, the prover's and the verifier's fixed points.
func hipGroth16FromCrs(crs C.ps_groth16_crs, q *HipQAP) *HipGroth16 {
	hs := &HipGroth16{qap: q, xi: crs.xi, xi2: crs.xi2, nioLP: crs.nio_lp, xiT: crs.xi_t, ioLP: crs.io_lp, crs: crs}
	hs.lagrange = []*C.ps_points{crs.lxi, crs.lxi2, crs.lxi_t}
	hs.pk.alpha, hs.pk.beta, hs.pk.delta, hs.pk.beta2, hs.pk.delta2 = crs.alpha, crs.beta, crs.delta, crs.beta2, crs.delta2
	hs.pk.xi, hs.pk.xi2, hs.pk.nio_lp, hs.pk.xi_t = crs.xi, crs.xi2, crs.nio_lp, crs.xi_t
	hs.pk.lxi, hs.pk.lxi2, hs.pk.lxi_t = crs.lxi, crs.lxi2, crs.lxi_t
	hs.vk.alpha, hs.vk.beta2, hs.vk.gamma, hs.vk.delta2 = crs.alpha, crs.beta2, crs.gamma, crs.delta2
	hs.vk.io_lp = crs.io_lp
	return hs
}

// NewHipGroth16FromSRS derives the circuit's key from the string alone (ps_groth16_setup_from_srs): the key
// NewGroth16TrustedSetup makes for the same alpha, beta, x and delta = gamma = 1, in both forms.  A wrong array length
// panics like BlindEval (algebra.go:350-352).
func NewHipGroth16FromSRS(srs Groth16SRS, q *HipQAP) *HipGroth16 {
	var s C.ps_groth16_srs
	s.tau_g1 = uploadPoints(C.PS_G1, srs.TauG1)
	s.tau_g2 = uploadPoints(C.PS_G2, srs.TauG2)
	s.alpha_tau_g1 = uploadPoints(C.PS_G1, srs.AlphaTauG1)
	s.beta_tau_g1 = uploadPoints(C.PS_G1, srs.BetaTauG1)
	defer func() {
		for _, p := range []*C.ps_points{s.tau_g1, s.tau_g2, s.alpha_tau_g1, s.beta_tau_g1} {
			C.ps_points_free(p)
		}
	}()
	copyTo(unsafe.Pointer(&s.beta_g2[0]), affineOf(C.PS_G2, srs.BetaG2))
	var crs C.ps_groth16_crs
	call(func() C.int { return C.ps_groth16_setup_from_srs(hipCtx, q.h, &s, &crs) })
	return hipGroth16FromCrs(crs, q)
}

// ContributeHIP folds a share into the key: delta *= d, gamma *= g (ps_groth16_crs_contribute).  d and g are drawn by the
// caller and must be forgotten afterwards.  The result shares Xi, Xi2 and their Lagrange forms with hs (reference
// counted); both are Free()d as usual.  Only keys made by NewHipGroth16FromSRS or ContributeHIP carry what this needs.
func (hs *HipGroth16) ContributeHIP(d, g Element) *HipGroth16 {
	db, err := d.MarshalBinary()
	if err != nil {
		panic(err)
	}
	gb, err := g.MarshalBinary()
	if err != nil {
		panic(err)
	}
	var out C.ps_groth16_crs
	call(func() C.int { return C.ps_groth16_crs_contribute(hipCtx, &hs.crs, u8(db), u8(gb), &out) })
	return hipGroth16FromCrs(out, hs.qap)
}

// CheckUpdateHIP: was `after` made from `before` by folding in SOME shares (ps_groth16_crs_check_update)?  The weights of
// the random linear combinations are drawn here, after both keys are in hand, 128 bits each.
func CheckUpdateHIP(before, after *HipGroth16) bool {
	n := 0
	for _, p := range []*C.ps_points{before.nioLP, before.xiT, before.ioLP} {
		if l := int(C.ps_points_len(p)); l > n {
			n = l
		}
	}
	rho := make([]byte, 32*n)
	for i := 0; i < n; i++ {
		random.Bytes(rho[32*i+16:32*i+32], random.New())
	}
	var ok C.int
	call(func() C.int {
		return C.ps_groth16_crs_check_update(hipCtx, &before.crs, &after.crs, u8(rho), C.size_t(n), &ok)
	})
	return ok != 0
}

// ---------------------------------------------------------------------------------------
// Phase 1: making and checking the string itself.  A ceremony starts from the trivial string (every point a generator),
// every party folds a share (t, a, b) of its own into tau, alpha, beta and publishes (t G2, a G2, b G2), and anybody checks
// every fold.  That a contributor KNOWS its t, a, b is for the ceremony protocol to establish, not for these calls.
// ---------------------------------------------------------------------------------------

// HipGroth16SRS is a phase-1 string resident on the device: folds and checks run on it without crossing the host.
type HipGroth16SRS struct {
	s C.ps_groth16_srs
}

// Groth16SRSShare holds a contributor's public values t G2, a G2, b G2.
type Groth16SRSShare struct {
	T2, A2, B2 Commit
}

// UploadGroth16SRS puts a string on the device.  Free() it when done.
func UploadGroth16SRS(srs Groth16SRS) *HipGroth16SRS {
	h := &HipGroth16SRS{}
	h.s.tau_g1 = uploadPoints(C.PS_G1, srs.TauG1)
	h.s.tau_g2 = uploadPoints(C.PS_G2, srs.TauG2)
	h.s.alpha_tau_g1 = uploadPoints(C.PS_G1, srs.AlphaTauG1)
	h.s.beta_tau_g1 = uploadPoints(C.PS_G1, srs.BetaTauG1)
	copyTo(unsafe.Pointer(&h.s.beta_g2[0]), affineOf(C.PS_G2, srs.BetaG2))
	return h
}

// Free releases the four arrays.
func (h *HipGroth16SRS) Free() {
	for _, p := range []*C.ps_points{h.s.tau_g1, h.s.tau_g2, h.s.alpha_tau_g1, h.s.beta_tau_g1} {
		C.ps_points_free(p)
	}
	h.s = C.ps_groth16_srs{}
}

// PowersHIP returns [c, c s, .., c s^(n-1)] computed on the device (ps_scalars_powers).
func PowersHIP(s, c Element, n int) Poly {
	var h *C.ps_scalars
	call(func() C.int { return C.ps_scalars_powers(hipCtx, u8(mustMarshalElement(s)), u8(mustMarshalElement(c)), C.size_t(n), &h) })
	defer C.ps_scalars_free(h)
	return downloadPoly(h)
}

func mustMarshalElement(e Element) []byte {
	b, err := e.MarshalBinary()
	if err != nil {
		panic(err)
	}
	return b
}

// Groth16SRSContribute folds a share into the string: tau *= t, alpha *= a, beta *= b (ps_groth16_srs_contribute).  t, a
// and b are drawn by the caller and must be forgotten afterwards.  The result is a new string; both are Free()d.
func Groth16SRSContribute(in *HipGroth16SRS, t, a, b Element) (*HipGroth16SRS, Groth16SRSShare) {
	out := &HipGroth16SRS{}
	var sh C.ps_groth16_srs_share
	call(func() C.int {
		return C.ps_groth16_srs_contribute(hipCtx, &in.s, u8(mustMarshalElement(t)), u8(mustMarshalElement(a)),
			u8(mustMarshalElement(b)), &out.s, &sh)
	})
	g2 := func(p *C.uint8_t) Commit { return pointFrom(C.PS_G2, bytesOf(unsafe.Pointer(p), g2Wire), zeroG2) }
	return out, Groth16SRSShare{T2: g2(&sh.t_g2[0]), A2: g2(&sh.a_g2[0]), B2: g2(&sh.b_g2[0])}
}

// srsWeights draws one 128-bit weight per neighbouring pair of the longest array, after the string is in hand.
func srsWeights(srs *HipGroth16SRS) ([]byte, int) {
	n := 0
	for _, p := range []*C.ps_points{srs.s.tau_g1, srs.s.tau_g2, srs.s.alpha_tau_g1, srs.s.beta_tau_g1} {
		if l := int(C.ps_points_len(p)); l > n {
			n = l
		}
	}
	rho := make([]byte, 32*n)
	for i := 0; i < n; i++ {
		random.Bytes(rho[32*i+16:32*i+32], random.New())
	}
	return rho, n
}

// Groth16SRSCheck: is the string well formed -- the powers of one tau in both groups, the same tau under alpha and beta,
// the same beta in G2 (ps_groth16_srs_check)?  checkSubgroup = false only for a string this process made itself.
func Groth16SRSCheck(srs *HipGroth16SRS, checkSubgroup bool) bool {
	rho, n := srsWeights(srs)
	sub := C.int(0)
	if checkSubgroup {
		sub = 1
	}
	var ok C.int
	call(func() C.int { return C.ps_groth16_srs_check(hipCtx, &srs.s, u8(rho), C.size_t(n), sub, &ok) })
	return ok != 0
}

// Groth16SRSCheckUpdate: is `after` well formed and `before` with the (t, a, b) behind `share` folded in
// (ps_groth16_srs_check_update)?  `before` is taken as checked.
func Groth16SRSCheckUpdate(before, after *HipGroth16SRS, share Groth16SRSShare) bool {
	var sh C.ps_groth16_srs_share
	copyTo(unsafe.Pointer(&sh.t_g2[0]), affineOf(C.PS_G2, share.T2))
	copyTo(unsafe.Pointer(&sh.a_g2[0]), affineOf(C.PS_G2, share.A2))
	copyTo(unsafe.Pointer(&sh.b_g2[0]), affineOf(C.PS_G2, share.B2))
	rho, n := srsWeights(after)
	var ok C.int
	call(func() C.int {
		return C.ps_groth16_srs_check_update(hipCtx, &before.s, &after.s, &sh, u8(rho), C.size_t(n), &ok)
	})
	return ok != 0
}

// drawWeights returns n weights of 128 random bits each, as n x 32 big-endian bytes.
func drawWeights(n int) []byte {
	rho := make([]byte, 32*n)
	for i := 0; i < n; i++ {
		random.Bytes(rho[32*i+16:32*i+32], random.New())
	}
	return rho
}

// CheckFromSRSHIP: is `key` what NewHipGroth16FromSRS(srs, q) makes, with SOME shares folded in (none, one ContributeHIP or
// several) -- without deriving it again (ps_groth16_crs_check_from_srs)?  The last link of the ceremony chain: sums over the
// string with interpolated weights and four pairing equalities in place of five conversions over group elements.  The
// weights are drawn here, after string and key are in hand.  checkSubgroup = false only for a key this process made itself.
func CheckFromSRSHIP(srs *HipGroth16SRS, key *HipGroth16, checkSubgroup bool) bool {
	q := key.qap
	n := q.nbVars
	if q.nbGates > n {
		n = q.nbGates
	}
	rho := drawWeights(n)
	sub := C.int(0)
	if checkSubgroup {
		sub = 1
	}
	var ok C.int
	call(func() C.int {
		return C.ps_groth16_crs_check_from_srs(hipCtx, q.h, &srs.s, &key.crs, u8(rho), C.size_t(n), sub, &ok)
	})
	return ok != 0
}

// ---------------------------------------------------------------------------------------
// KZG commitments over the string's tau_g1: Poly.Commit / PolyCommit, Poly.Eval (algebra.go:107-115) and Poly.Div by a
// linear factor (algebra.go:119-137)
// ---------------------------------------------------------------------------------------

func uploadPoly(p Poly) *C.ps_scalars {
	var h *C.ps_scalars
	raw := marshalScalars(p)
	call(func() C.int { return C.ps_scalars_upload(hipCtx, u8(raw), C.size_t(len(p)), &h) })
	return h
}

func elementsFrom(raw []byte) []Element {
	out := make([]Element, len(raw)/32)
	for i := range out {
		e := NewElement()
		if err := e.UnmarshalBinary(raw[32*i : 32*i+32]); err != nil {
			panic(err)
		}
		out[i] = e
	}
	return out
}

// PolyScanTile is the number of coefficients one workgroup of the device scan owns (ps_poly_scan_tile).
func PolyScanTile() int { return int(C.ps_poly_scan_tile()) }

// EvalHIP replaces `func (p Poly) Eval(i Element) Element` for several points at once (ps_poly_eval).
func (p Poly) EvalHIP(zs []Element) []Element {
	h := uploadPoly(p)
	defer C.ps_scalars_free(h)
	ys := make([]byte, 32*len(zs))
	call(func() C.int { return C.ps_poly_eval(hipCtx, h, u8(marshalScalars(Poly(zs))), C.size_t(len(zs)), u8(ys)) })
	return elementsFrom(ys)
}

// DivLinearHIP replaces `func (p Poly) Div(p2 Poly)` for the divisors (X - z), z in zs: the quotients, lowest degree first,
// and the remainders p(z) (ps_poly_div_linear).
func (p Poly) DivLinearHIP(zs []Element) ([]Poly, []Element) {
	h := uploadPoly(p)
	defer C.ps_scalars_free(h)
	var q *C.ps_scalars
	rem := make([]byte, 32*len(zs))
	call(func() C.int { return C.ps_poly_div_linear(hipCtx, h, u8(marshalScalars(Poly(zs))), C.size_t(len(zs)), &q, u8(rem)) })
	defer C.ps_scalars_free(q)
	all := downloadPoly(q)
	rows := make([]Poly, len(zs))
	for j := range rows {
		rows[j] = all[j*(len(p)-1) : (j+1)*(len(p)-1)]
	}
	return rows, elementsFrom(rem)
}

// KZGCommit replaces `func (p Poly) Commit`: [p(tau)] G1 over the string's first len(p) powers (ps_kzg_commit).
func KZGCommit(srs *HipGroth16SRS, p Poly) Commit {
	h := uploadPoly(p)
	defer C.ps_scalars_free(h)
	out := make([]byte, g1Wire)
	call(func() C.int { return C.ps_kzg_commit(hipCtx, srs.s.tau_g1, h, u8(out)) })
	return pointFrom(C.PS_G1, out, zeroG1)
}

// KZGOpen returns p(z) and the opening proof [q_z(tau)] G1 for every z in zs (ps_kzg_open).
func KZGOpen(srs *HipGroth16SRS, p Poly, zs []Element) ([]Element, []Commit) {
	h := uploadPoly(p)
	defer C.ps_scalars_free(h)
	ys := make([]byte, 32*len(zs))
	raw := make([]byte, g1Wire*len(zs))
	call(func() C.int {
		return C.ps_kzg_open(hipCtx, srs.s.tau_g1, h, u8(marshalScalars(Poly(zs))), C.size_t(len(zs)), u8(ys), u8(raw))
	})
	proofs := make([]Commit, len(zs))
	for j := range proofs {
		proofs[j] = pointFrom(C.PS_G1, raw[g1Wire*j:g1Wire*(j+1)], zeroG1)
	}
	return elementsFrom(ys), proofs
}

// tauG2 fetches tau G2 = tau_g2[1] of the string, affine.
func tauG2(srs *HipGroth16SRS) []byte {
	out := make([]byte, g2Wire)
	call(func() C.int { return C.ps_points_download(hipCtx, srs.s.tau_g2, 1, 1, u8(out)) })
	return out
}

// KZGVerify checks one opening: e(C - y G1 + z pi, G2) == e(pi, tau G2), on the host (ps_kzg_verify).
func KZGVerify(srs *HipGroth16SRS, commit Commit, z, y Element, proof Commit) bool {
	t2 := tauG2(srs)
	var ok C.int
	check(func() C.int {
		return C.ps_kzg_verify(u8(t2), u8(affineOf(C.PS_G1, commit)), u8(mustMarshalElement(z)), u8(mustMarshalElement(y)),
			u8(affineOf(C.PS_G1, proof)), &ok)
	})
	return ok != 0
}

// KZGVerifyBatch checks len(commits) openings under one string in one weighted equation (ps_kzg_verify_batch).  The weights
// are drawn here, after everything else is in hand.  checkSubgroup = false only for points this process made itself.
func KZGVerifyBatch(srs *HipGroth16SRS, commits []Commit, zs, ys []Element, proofs []Commit, checkSubgroup bool) bool {
	k := len(commits)
	if len(zs) != k || len(ys) != k || len(proofs) != k {
		panic(fmt.Sprintf("KZGVerifyBatch: %d commitments, %d points, %d values, %d proofs", k, len(zs), len(ys), len(proofs)))
	}
	t2 := tauG2(srs)
	cs, ps := make([]byte, 0, g1Wire*k), make([]byte, 0, g1Wire*k)
	for j := 0; j < k; j++ {
		cs = append(cs, affineOf(C.PS_G1, commits[j])...)
		ps = append(ps, affineOf(C.PS_G1, proofs[j])...)
	}
	rho := drawWeights(k)
	sub := C.int(0)
	if checkSubgroup {
		sub = 1
	}
	var ok C.int
	call(func() C.int {
		return C.ps_kzg_verify_batch(hipCtx, u8(t2), u8(cs), u8(marshalScalars(Poly(zs))), u8(marshalScalars(Poly(ys))), u8(ps), u8(rho),
			C.size_t(k), sub, &ok)
	})
	return ok != 0
}

// LinCombHIP returns the len(coef[0]) rows sum_i coef[i][j] * polys[i], every polynomial zero-extended to the longest
// (ps_scalars_lincomb).  `func (p Poly) Add` / `Sub` (algebra.go:161-196) are the columns (1, 1) and (1, -1); the rows are not
// normalised.
func LinCombHIP(polys []Poly, coef [][]Element) []Poly {
	m := len(polys)
	if m == 0 || len(coef) != m {
		panic(fmt.Sprintf("LinCombHIP: %d polynomials, %d rows of coefficients", m, len(coef)))
	}
	t := len(coef[0])
	hs := make([]*C.ps_scalars, m)
	flat := make(Poly, 0, m*t)
	n := 0
	for i, p := range polys {
		hs[i] = uploadPoly(p)
		defer C.ps_scalars_free(hs[i])
		flat = append(flat, coef[i]...)
		if len(p) > n {
			n = len(p)
		}
	}
	var out *C.ps_scalars
	call(func() C.int {
		return C.ps_scalars_lincomb(hipCtx, (**C.ps_scalars)(unsafe.Pointer(&hs[0])), C.size_t(m), u8(marshalScalars(flat)), C.size_t(t), &out)
	})
	defer C.ps_scalars_free(out)
	all := downloadPoly(out)
	rows := make([]Poly, t)
	for j := range rows {
		rows[j] = all[j*n : (j+1)*n]
	}
	return rows
}

// KZGOpenMulti opens len(polys) polynomials at len(zs) points with ONE proof per point (ps_kzg_open_multi).  coef[i][j] != 0
// means "polynomial i is opened at point j, with this weight": powers of a Fiat-Shamir challenge drawn after the commitments
// and the values are fixed.  ys[i][j] = polys[i](zs[j]) where coef[i][j] != 0 and zero elsewhere.
func KZGOpenMulti(srs *HipGroth16SRS, polys []Poly, zs []Element, coef [][]Element) ([][]Element, []Commit) {
	m, t := len(polys), len(zs)
	if m == 0 || len(coef) != m {
		panic(fmt.Sprintf("KZGOpenMulti: %d polynomials, %d rows of coefficients", m, len(coef)))
	}
	hs := make([]*C.ps_scalars, m)
	flat := make(Poly, 0, m*t)
	for i, p := range polys {
		hs[i] = uploadPoly(p)
		defer C.ps_scalars_free(hs[i])
		flat = append(flat, coef[i]...)
	}
	ys := make([]byte, 32*m*t)
	raw := make([]byte, g1Wire*t)
	call(func() C.int {
		return C.ps_kzg_open_multi(hipCtx, srs.s.tau_g1, (**C.ps_scalars)(unsafe.Pointer(&hs[0])), C.size_t(m), u8(marshalScalars(Poly(zs))),
			C.size_t(t), u8(marshalScalars(flat)), u8(ys), u8(raw))
	})
	vals := elementsFrom(ys)
	rows := make([][]Element, m)
	for i := range rows {
		rows[i] = vals[i*t : (i+1)*t]
	}
	proofs := make([]Commit, t)
	for j := range proofs {
		proofs[j] = pointFrom(C.PS_G1, raw[g1Wire*j:g1Wire*(j+1)], zeroG1)
	}
	return rows, proofs
}

// KZGVerifyMulti checks what KZGOpenMulti made in one weighted equation (ps_kzg_verify_multi).  The weights of the points are
// drawn here, after everything else is in hand.
func KZGVerifyMulti(srs *HipGroth16SRS, commits []Commit, zs []Element, coef, ys [][]Element, proofs []Commit, checkSubgroup bool) bool {
	m, t := len(commits), len(zs)
	if len(coef) != m || len(ys) != m || len(proofs) != t {
		panic(fmt.Sprintf("KZGVerifyMulti: %d commitments, %d points, %d rows of weights, %d of values, %d proofs", m, t, len(coef), len(ys), len(proofs)))
	}
	t2 := tauG2(srs)
	cs, ps := make([]byte, 0, g1Wire*m), make([]byte, 0, g1Wire*t)
	cf, yf := make(Poly, 0, m*t), make(Poly, 0, m*t)
	for i := 0; i < m; i++ {
		cs = append(cs, affineOf(C.PS_G1, commits[i])...)
		cf = append(cf, coef[i]...)
		yf = append(yf, ys[i]...)
	}
	for j := 0; j < t; j++ {
		ps = append(ps, affineOf(C.PS_G1, proofs[j])...)
	}
	rho := drawWeights(t)
	sub := C.int(0)
	if checkSubgroup {
		sub = 1
	}
	var ok C.int
	call(func() C.int {
		return C.ps_kzg_verify_multi(hipCtx, u8(t2), u8(cs), C.size_t(m), u8(marshalScalars(Poly(zs))), C.size_t(t), u8(marshalScalars(cf)),
			u8(marshalScalars(yf)), u8(ps), u8(rho), sub, &ok)
	})
	return ok != 0
}

// PolyScanSetGroup is the number of points one workgroup of the set apply pass folds (ps_poly_scan_set_group).
func PolyScanSetGroup() int { return int(C.ps_poly_scan_set_group()) }

// DivRootsHIP replaces `func (p Poly) Div(p2 Poly)` for the divisor Z_S = prod (X - z), z in zs, at least one and all distinct
// (ps_poly_div_roots): the len(p) - len(zs) quotient coefficients, lowest degree first (none for len(p) <= len(zs)), the values
// p(z), and the len(zs) coefficients of the remainder -- the interpolant of (z, p(z)).
func (p Poly) DivRootsHIP(zs []Element) (Poly, []Element, Poly) {
	h := uploadPoly(p)
	defer C.ps_scalars_free(h)
	var q *C.ps_scalars
	ys := make([]byte, 32*len(zs))
	rem := make([]byte, 32*len(zs))
	call(func() C.int {
		return C.ps_poly_div_roots(hipCtx, h, u8(marshalScalars(Poly(zs))), C.size_t(len(zs)), &q, u8(ys), u8(rem))
	})
	defer C.ps_scalars_free(q)
	quot := Poly{}
	if len(p) > len(zs) {
		quot = downloadPoly(q)
	}
	return quot, elementsFrom(ys), Poly(elementsFrom(rem))
}

// KZGOpenSet returns the values p(z), z in zs, and ONE proof [q(tau)] G1 for the whole set, q = (p - r) / prod (X - z) with r
// the interpolant of the values (ps_kzg_open_set).  At least one point, all distinct.
func KZGOpenSet(srs *HipGroth16SRS, p Poly, zs []Element) ([]Element, Commit) {
	h := uploadPoly(p)
	defer C.ps_scalars_free(h)
	ys := make([]byte, 32*len(zs))
	raw := make([]byte, g1Wire)
	call(func() C.int {
		return C.ps_kzg_open_set(hipCtx, srs.s.tau_g1, h, u8(marshalScalars(Poly(zs))), C.size_t(len(zs)), u8(ys), u8(raw))
	})
	return elementsFrom(ys), pointFrom(C.PS_G1, raw, zeroG1)
}

// KZGVerifySet checks what KZGOpenSet made: e(C - [r(tau)] G1, G2) e(-pi, [Z_S(tau)] G2) == 1 (ps_kzg_verify_set).  The string
// holds at least len(zs) powers in G1 and len(zs) + 1 in G2.  checkSubgroup = false only for points this process made itself.
func KZGVerifySet(srs *HipGroth16SRS, commit Commit, zs, ys []Element, proof Commit, checkSubgroup bool) bool {
	if len(zs) != len(ys) {
		panic(fmt.Sprintf("KZGVerifySet: %d points, %d values", len(zs), len(ys)))
	}
	sub := C.int(0)
	if checkSubgroup {
		sub = 1
	}
	var ok C.int
	call(func() C.int {
		return C.ps_kzg_verify_set(hipCtx, srs.s.tau_g1, srs.s.tau_g2, u8(affineOf(C.PS_G1, commit)), u8(marshalScalars(Poly(zs))),
			u8(marshalScalars(Poly(ys))), C.size_t(len(zs)), u8(affineOf(C.PS_G1, proof)), sub, &ok)
	})
	return ok != 0
}

// ---------------------------------------------------------------------------------------
// KZG over polynomials held as their VALUES on the domain 1..n of a HipQAP (the Lagrange form): what a prover has -- the gate
// vectors L.w, R.w, O.w, a column, a blob -- committed and opened with no interpolation and no division.  Commitments and proofs
// are the group elements KZGCommit and KZGOpen give for the interpolated coefficients, so KZGVerify checks them unchanged.
// ---------------------------------------------------------------------------------------

// PolyLagrangeTile is the number of nodes one workgroup inverts together (ps_poly_lagrange_tile).
func PolyLagrangeTile() int { return int(C.ps_poly_lagrange_tile()) }

// GateValuesHIP returns the nbGates values of (L|R|O).sol on the domain, which = 0, 1, 2: what computeAggregatePoly
// (qap.go:164-175) interpolates, uninterpolated (ps_qap_gate_values).
func (q *HipQAP) GateValuesHIP(sol Vector, which int) Poly {
	dsol := uploadSolution(sol)
	defer C.ps_scalars_free(dsol)
	var h *C.ps_scalars
	call(func() C.int { return C.ps_qap_gate_values(hipCtx, q.h, dsol, C.int(which), &h) })
	defer C.ps_scalars_free(h)
	return downloadPoly(h)
}

// LagrangeStringHIP puts the first nbGates powers of the string's tau_g1 into Lagrange form on the domain
// (ps_points_monomial_to_lagrange, once per string and domain): the array KZGCommitLagrange and KZGOpenLagrange sum over.
// The caller frees it with ps_points_free.
func (q *HipQAP) LagrangeStringHIP(srs *HipGroth16SRS) *C.ps_points {
	var head, lag *C.ps_points
	call(func() C.int { return C.ps_points_slice(srs.s.tau_g1, 0, C.size_t(q.nbGates), &head) })
	defer C.ps_points_free(head)
	call(func() C.int { return C.ps_points_monomial_to_lagrange(hipCtx, q.h, head, 0, &lag) })
	return lag
}

// EvalLagrangeHIP is EvalHIP for a polynomial held as its nbGates values on the domain (ps_poly_eval_lagrange).  Points may lie
// on the domain.
func (q *HipQAP) EvalLagrangeHIP(values Poly, zs []Element) []Element {
	h := uploadPoly(values)
	defer C.ps_scalars_free(h)
	ys := make([]byte, 32*len(zs))
	call(func() C.int {
		return C.ps_poly_eval_lagrange(hipCtx, q.h, h, u8(marshalScalars(Poly(zs))), C.size_t(len(zs)), u8(ys))
	})
	return elementsFrom(ys)
}

// DivLinearLagrangeHIP is DivLinearHIP in value form: row j holds the nbGates values on the domain of (p - p(z)) / (X - z),
// z = zs[j], next to the values p(z) (ps_poly_div_linear_lagrange).
func (q *HipQAP) DivLinearLagrangeHIP(values Poly, zs []Element) ([]Poly, []Element) {
	h := uploadPoly(values)
	defer C.ps_scalars_free(h)
	var qv *C.ps_scalars
	ys := make([]byte, 32*len(zs))
	call(func() C.int {
		return C.ps_poly_div_linear_lagrange(hipCtx, q.h, h, u8(marshalScalars(Poly(zs))), C.size_t(len(zs)), &qv, u8(ys))
	})
	defer C.ps_scalars_free(qv)
	rows := make([]Poly, len(zs))
	if len(zs) > 0 {
		all := downloadPoly(qv)
		for j := range rows {
			rows[j] = all[j*len(values) : (j+1)*len(values)]
		}
	}
	return rows, elementsFrom(ys)
}

// KZGCommitLagrange returns [p(tau)] G1 for the polynomial with the given values, over the Lagrange-form string
// (ps_kzg_commit_lagrange): the point KZGCommit gives for the interpolated coefficients.
func KZGCommitLagrange(lagG1 *C.ps_points, values Poly) Commit {
	h := uploadPoly(values)
	defer C.ps_scalars_free(h)
	out := make([]byte, g1Wire)
	call(func() C.int { return C.ps_kzg_commit_lagrange(hipCtx, lagG1, h, u8(out)) })
	return pointFrom(C.PS_G1, out, zeroG1)
}

// KZGOpenLagrange returns p(z) and the opening proof [q_z(tau)] G1 for every z in zs from the values alone
// (ps_kzg_open_lagrange): the points KZGOpen gives for the interpolated coefficients.
func KZGOpenLagrange(q *HipQAP, lagG1 *C.ps_points, values Poly, zs []Element) ([]Element, []Commit) {
	h := uploadPoly(values)
	defer C.ps_scalars_free(h)
	ys := make([]byte, 32*len(zs))
	raw := make([]byte, g1Wire*len(zs))
	call(func() C.int {
		return C.ps_kzg_open_lagrange(hipCtx, q.h, lagG1, h, u8(marshalScalars(Poly(zs))), C.size_t(len(zs)), u8(ys), u8(raw))
	})
	proofs := make([]Commit, len(zs))
	for j := range proofs {
		proofs[j] = pointFrom(C.PS_G1, raw[g1Wire*j:g1Wire*(j+1)], zeroG1)
	}
	return elementsFrom(ys), proofs
}

// PolyLagrangeSetGroup is the number of points of a set that share one inversion per tile (ps_poly_lagrange_set_group).
func PolyLagrangeSetGroup() int { return int(C.ps_poly_lagrange_set_group()) }

// DivRootsLagrangeHIP is DivRootsHIP in value form: the nbGates values on the domain of (p - r) / prod (X - z), z in zs (all
// zero for len(zs) >= nbGates), the values p(z), and the len(zs) coefficients of the remainder r
// (ps_poly_div_roots_lagrange).  At least one point, all distinct, on the domain or off it.
func (q *HipQAP) DivRootsLagrangeHIP(values Poly, zs []Element) (Poly, []Element, Poly) {
	h := uploadPoly(values)
	defer C.ps_scalars_free(h)
	var qv *C.ps_scalars
	ys := make([]byte, 32*len(zs))
	rem := make([]byte, 32*len(zs))
	call(func() C.int {
		return C.ps_poly_div_roots_lagrange(hipCtx, q.h, h, u8(marshalScalars(Poly(zs))), C.size_t(len(zs)), &qv, u8(ys), u8(rem))
	})
	defer C.ps_scalars_free(qv)
	return downloadPoly(qv), elementsFrom(ys), Poly(elementsFrom(rem))
}

// KZGOpenSetLagrange returns the values p(z), z in zs, and ONE proof for the whole set from the values alone
// (ps_kzg_open_set_lagrange): the point KZGOpenSet gives for the interpolated coefficients, which KZGVerifySet checks unchanged.
func KZGOpenSetLagrange(q *HipQAP, lagG1 *C.ps_points, values Poly, zs []Element) ([]Element, Commit) {
	h := uploadPoly(values)
	defer C.ps_scalars_free(h)
	ys := make([]byte, 32*len(zs))
	raw := make([]byte, g1Wire)
	call(func() C.int {
		return C.ps_kzg_open_set_lagrange(hipCtx, q.h, lagG1, h, u8(marshalScalars(Poly(zs))), C.size_t(len(zs)), u8(ys), u8(raw))
	})
	return elementsFrom(ys), pointFrom(C.PS_G1, raw, zeroG1)
}

// KZGAllKeyLagrange returns K_m = sum_i lagG1[i-1] / (m - i), m = 1..nbGates, on the device (ps_kzg_all_key_lagrange): the part
// of the proofs of all nodes that depends on the domain and the string alone.  The caller frees it with ps_points_free.
func KZGAllKeyLagrange(q *HipQAP, lagG1 *C.ps_points) *C.ps_points {
	var key *C.ps_points
	call(func() C.int { return C.ps_kzg_all_key_lagrange(hipCtx, q.h, lagG1, &key) })
	return key
}

// KZGOpenAllLagrange returns the opening proofs of EVERY node of the domain, element m - 1 for the node m, from the values alone
// (ps_kzg_open_all_lagrange): the points KZGOpenLagrange gives at z = 1..nbGates, from two transforms over points instead of
// nbGates sums.  allKey is what KZGAllKeyLagrange returned for (q, lagG1), or nil (computed inside the call and dropped).
func KZGOpenAllLagrange(q *HipQAP, lagG1, allKey *C.ps_points, values Poly) []Commit {
	h := uploadPoly(values)
	defer C.ps_scalars_free(h)
	var dev *C.ps_points
	call(func() C.int { return C.ps_kzg_open_all_lagrange(hipCtx, q.h, lagG1, allKey, h, &dev) })
	defer C.ps_points_free(dev)
	n := int(C.ps_points_len(dev))
	raw := make([]byte, g1Wire*maxInt(n, 1))
	call(func() C.int { return C.ps_points_download(hipCtx, dev, 0, C.size_t(n), u8(raw)) })
	proofs := make([]Commit, n)
	for m := range proofs {
		proofs[m] = pointFrom(C.PS_G1, raw[g1Wire*m:g1Wire*(m+1)], zeroG1)
	}
	return proofs
}

// LagrangeCheckHIP: are the Lagrange-form arrays of the key what ToLagrange() makes of its monomial ones, without making
// them (ps_points_lagrange_check, once per array)?  False for a key that has no Lagrange form.
func (hs *HipGroth16) LagrangeCheckHIP() bool {
	if hs.pk.lxi == nil || hs.pk.lxi2 == nil || hs.pk.lxi_t == nil {
		return false
	}
	n := hs.qap.nbGates
	rho := drawWeights(n)
	pairs := []struct {
		mono, lagr *C.ps_points
		nodes      C.int
	}{{hs.xi, hs.pk.lxi, 0}, {hs.xi2, hs.pk.lxi2, 0}, {hs.xiT, hs.pk.lxi_t, 1}}
	for _, p := range pairs {
		var ok C.int
		call(func() C.int {
			return C.ps_points_lagrange_check(hipCtx, hs.qap.h, p.mono, p.lagr, p.nodes, u8(rho), C.size_t(n), &ok)
		})
		if ok == 0 {
			return false
		}
	}
	return true
}

// ---------------------------------------------------------------------------------------
// Several GPUs from ONE process (a cgo caller cannot wrap a function call in one process per GPU, which is how
// bench.py and playsnark_amd/dist.py scale): ps_msm_multi_device and ps_groth16_prove_multi run one context per
// device side by side and fold the per-device partial sums on the host (SURVEY.md 8e, DESIGN.md section 7).
// ---------------------------------------------------------------------------------------

// shardRange is the index range [first, first+count) of device d of ndev: contiguous, sizes differ by at most one
// (the split ps_groth16_prove_multi checks with PS_ERR_LENGTH).
func shardRange(n, d, ndev int) (int, int) {
	base, extra := n/ndev, n%ndev
	first := d*base + minInt(d, extra)
	if d < extra {
		return first, base + 1
	}
	return first, base
}

func minInt(a, b int) int {
	if a < b {
		return a
	}
	return b
}

// HipDevices is one context per GPU of this process.
type HipDevices struct {
	mu   sync.Mutex
	ctxs []*C.ps_ctx
}

func NewHipDevices(ndev int) *HipDevices {
	hd := &HipDevices{}
	for d := 0; d < ndev; d++ {
		var c *C.ps_ctx
		check(func() C.int { return C.ps_ctx_create(C.int(d), &c) })
		hd.ctxs = append(hd.ctxs, c)
	}
	return hd
}

func (hd *HipDevices) Free() {
	for _, c := range hd.ctxs {
		C.ps_ctx_destroy(c)
	}
}

// HipShardedPoints is a CRS slice cut by index range over the devices (device d holds shardRange(len, d, ndev)).
type HipShardedPoints struct {
	parts []*C.ps_points
	n     int
}

func (hd *HipDevices) UploadPoints(group C.int, pts []Commit) *HipShardedPoints {
	sp := &HipShardedPoints{n: len(pts)}
	for d, c := range hd.ctxs {
		first, cnt := shardRange(len(pts), d, len(hd.ctxs))
		raw := marshalPoints(pts[first : first+cnt])
		var h *C.ps_points
		cc := c
		check(func() C.int { return C.ps_points_upload(cc, group, u8(raw), C.size_t(cnt), C.PS_FMT_COMPRESSED, &h) })
		sp.parts = append(sp.parts, h)
	}
	return sp
}

func (sp *HipShardedPoints) Free() {
	for _, p := range sp.parts {
		C.ps_points_free(p)
	}
}

// BlindEvalHIPMulti is Poly.BlindEval (algebra.go:348-359) with the sum sharded over the devices.
func (p Poly) BlindEvalHIPMulti(zero Commit, hd *HipDevices, crs *HipShardedPoints) Commit {
	if crs.n != len(p) { // algebra.go:350-352
		panic(fmt.Sprintf("mismatch of length between poly %d and blinded eval points %d", len(p), crs.n))
	}
	hd.mu.Lock()
	defer hd.mu.Unlock()
	ndev := len(hd.ctxs)
	scal := make([]*C.ps_scalars, ndev)
	for d, c := range hd.ctxs {
		first, cnt := shardRange(len(p), d, ndev)
		raw := marshalScalars(p[first : first+cnt])
		cc, dd := c, d
		check(func() C.int { return C.ps_scalars_upload(cc, u8(raw), C.size_t(cnt), &scal[dd]) })
		defer C.ps_scalars_free(scal[d])
	}
	group := C.ps_points_group(crs.parts[0])
	out := make([]byte, wireLen(group))
	// the three pointer arrays live in C memory (cgo: no Go pointers to Go pointers across the boundary)
	arr := func(n int) unsafe.Pointer { return C.malloc(C.size_t(n) * C.size_t(unsafe.Sizeof(uintptr(0)))) }
	cctx, cpts, csc := arr(ndev), arr(ndev), arr(ndev)
	defer C.free(cctx)
	defer C.free(cpts)
	defer C.free(csc)
	for d := 0; d < ndev; d++ {
		(*[1 << 20]*C.ps_ctx)(cctx)[d] = hd.ctxs[d]
		(*[1 << 20]*C.ps_points)(cpts)[d] = crs.parts[d]
		(*[1 << 20]*C.ps_scalars)(csc)[d] = scal[d]
	}
	check(func() C.int {
		return C.ps_msm_multi_device((**C.ps_ctx)(cctx), (**C.ps_points)(cpts), (**C.ps_scalars)(csc), C.size_t(ndev), u8(out))
	})
	return pointFrom(group, out, zero)
}

// HipGroth16Multi: every device holds only ITS index range of Xi, Xi2, NioLP, XiT (an eighth of the key on eight GPUs),
// its own QAP of the circuit and its own copy of the solution.
type HipGroth16Multi struct {
	hd     *HipDevices
	dev    []C.ps_groth16_device
	qaps   []*C.ps_qap
	arrays []*HipShardedPoints
}

func NewHipGroth16Multi(hd *HipDevices, tr Groth16Setup, circuit R1CS) *HipGroth16Multi {
	hm := &HipGroth16Multi{hd: hd, dev: make([]C.ps_groth16_device, len(hd.ctxs))} // zero-initialised, as the header requires
	xi, xi2 := hd.UploadPoints(C.PS_G1, tr.Xi), hd.UploadPoints(C.PS_G2, tr.Xi2)
	nio, xit := hd.UploadPoints(C.PS_G1, tr.NioLP), hd.UploadPoints(C.PS_G1, tr.XiT)
	hm.arrays = []*HipShardedPoints{xi, xi2, nio, xit}
	l, r, o := newCsr(circuit.left), newCsr(circuit.right), newCsr(circuit.out)
	defer l.free()
	defer r.free()
	defer o.free()
	// check() panics on a library error: a device that fails after others succeeded must not leak their QAPs and shards
	done := false
	defer func() {
		if !done {
			hm.Free()
		}
	}()
	for d, c := range hd.ctxs {
		var q *C.ps_qap
		cc := c
		check(func() C.int {
			return C.ps_qap_create(cc, C.size_t(len(circuit.left)), C.size_t(len(circuit.vars)), C.size_t(circuit.nbIO()), &l.csr, &r.csr, &o.csr, &q)
		})
		hm.qaps = append(hm.qaps, q)
		hm.dev[d].ctx, hm.dev[d].qap = c, q
		pk := &hm.dev[d].pk
		pk.xi, pk.xi2, pk.nio_lp, pk.xi_t = xi.parts[d], xi2.parts[d], nio.parts[d], xit.parts[d]
		if d == 0 { // the fixed points are read from dev[0].pk
			copyTo(unsafe.Pointer(&pk.alpha[0]), affineOf(C.PS_G1, tr.Alpha))
			copyTo(unsafe.Pointer(&pk.beta[0]), affineOf(C.PS_G1, tr.Beta))
			copyTo(unsafe.Pointer(&pk.delta[0]), affineOf(C.PS_G1, tr.Delta))
			copyTo(unsafe.Pointer(&pk.beta2[0]), affineOf(C.PS_G2, tr.Beta2))
			copyTo(unsafe.Pointer(&pk.delta2[0]), affineOf(C.PS_G2, tr.Delta2))
		}
	}
	done = true
	return hm
}

func (hm *HipGroth16Multi) Free() {
	for _, q := range hm.qaps {
		C.ps_qap_free(q)
	}
	for _, a := range hm.arrays {
		a.Free()
	}
}

// distributeDevicePoints cuts a device-resident array (on ctx `from`) by index range over the devices: device d gets
// shardRange(len, d, ndev) as an array of its own (downloaded once in affine form, uploaded per device).
func (hd *HipDevices) distributeDevicePoints(from *C.ps_ctx, src *C.ps_points) *HipShardedPoints {
	n := int(C.ps_points_len(src))
	group := C.ps_points_group(src)
	wire := g1Wire
	if group == C.PS_G2 {
		wire = g2Wire
	}
	raw := make([]byte, wire*maxInt(n, 1))
	check(func() C.int { return C.ps_points_download(from, src, 0, C.size_t(n), u8(raw)) })
	sp := &HipShardedPoints{n: n}
	for d, c := range hd.ctxs {
		first, cnt := shardRange(n, d, len(hd.ctxs))
		part := raw[first*wire : (first+cnt)*wire]
		if cnt == 0 {
			part = raw[:1] // never read: cnt is 0
		}
		var h *C.ps_points
		cc := c
		check(func() C.int { return C.ps_points_upload(cc, group, u8(part), C.size_t(cnt), C.PS_FMT_AFFINE, &h) })
		sp.parts = append(sp.parts, h)
	}
	return sp
}

func maxInt(a, b int) int {
	if a > b {
		return a
	}
	return b
}

// UseLagrange puts the multi-device key onto the route without coefficient vectors: hs is the same key on ONE device with its
// Lagrange form present (ToLagrange, or NewHipGroth16FromToxicWaste); its lxi, lxi2, lxi_t are cut by index range over the
// devices and handed to ps_groth16_prove_multi as the optional arrays of every device's pk.  From then on a proof moves
// 3 x 40 bytes per node of a device's range between devices and nothing through host memory (playsnark_hip.h).
func (hm *HipGroth16Multi) UseLagrange(hs *HipGroth16) {
	if hs.pk.lxi == nil || hs.pk.lxi2 == nil || hs.pk.lxi_t == nil {
		panic("playsnark_hip: UseLagrange needs a key with its Lagrange form (HipGroth16.ToLagrange)")
	}
	lxi := hm.hd.distributeDevicePoints(hipCtx, hs.pk.lxi)
	lxi2 := hm.hd.distributeDevicePoints(hipCtx, hs.pk.lxi2)
	lxit := hm.hd.distributeDevicePoints(hipCtx, hs.pk.lxi_t)
	hm.arrays = append(hm.arrays, lxi, lxi2, lxit)
	for d := range hm.dev { // on every device or on none (PS_ERR_ARG otherwise)
		pk := &hm.dev[d].pk
		pk.lxi, pk.lxi2, pk.lxi_t = lxi.parts[d], lxi2.parts[d], lxit.parts[d]
	}
}

// Groth16ProveHIPLocal is ONE rank's share of Groth16Prove when this process holds only its index ranges of a Lagrange-form
// key (one process per GPU; ps_groth16_prove_local): pk has lxi / lxi2 / lxi_t / nio_lp cut for (rank, world) and the fixed
// points, which the last rank adds.  The element-wise sum of all ranks' (A, B, C) is the proof of Groth16ProveHIP for the
// same (r, s); the caller gathers and adds them (Commit.Add).
func Groth16ProveHIPLocal(pk *C.ps_groth16_pk, qap *C.ps_qap, sol Vector, r, s Element, rank, world int) (Commit, Commit, Commit) {
	rb, _ := r.MarshalBinary()
	sb, _ := s.MarshalBinary()
	vals := make([]C.int64_t, len(sol))
	for i, v := range sol {
		vals[i] = C.int64_t(v)
	}
	var vp *C.int64_t
	if len(vals) > 0 {
		vp = &vals[0]
	}
	var h *C.ps_scalars
	check(func() C.int { return C.ps_scalars_upload_i64(hipCtx, vp, C.size_t(len(vals)), &h) })
	defer C.ps_scalars_free(h)
	A, B, Cc := make([]byte, g1Wire), make([]byte, g2Wire), make([]byte, g1Wire)
	check(func() C.int {
		return C.ps_groth16_prove_local(hipCtx, pk, qap, h, u8(rb), u8(sb), C.int(rank), C.int(world), u8(A), u8(B), u8(Cc))
	})
	return pointFrom(C.PS_G1, A, zeroG1), pointFrom(C.PS_G2, B, zeroG2), pointFrom(C.PS_G1, Cc, zeroG1)
}

// Groth16ProveHIPMulti is Groth16Prove (groth16.go:122-211) over the devices of this process: same proof bytes as
// Groth16ProveHIP for the same (r, s).  After UseLagrange the devices' pk carry lxi / lxi2 / lxi_t and the library takes the
// route without interpolation, division or host staging.
func Groth16ProveHIPMulti(hm *HipGroth16Multi, sol Vector) Groth16Proof {
	r := NewElement().Pick(random.New())
	s := NewElement().Pick(random.New())
	rb, _ := r.MarshalBinary()
	sb, _ := s.MarshalBinary()
	hm.hd.mu.Lock()
	defer hm.hd.mu.Unlock()
	vals := make([]C.int64_t, len(sol))
	for i, v := range sol {
		vals[i] = C.int64_t(v)
	}
	// the device structs go to C memory: they hold C pointers only, but live in a Go slice
	cdev := (*C.ps_groth16_device)(C.malloc(C.size_t(len(hm.dev)) * C.size_t(unsafe.Sizeof(hm.dev[0]))))
	defer C.free(unsafe.Pointer(cdev))
	devs := (*[1 << 16]C.ps_groth16_device)(unsafe.Pointer(cdev))[:len(hm.dev):len(hm.dev)]
	var vp *C.int64_t // an empty solution has no first element to point at (the library refuses it by length, not by a Go panic here)
	if len(vals) > 0 {
		vp = &vals[0]
	}
	for d := range hm.dev {
		var h *C.ps_scalars
		cc := hm.dev[d].ctx
		check(func() C.int { return C.ps_scalars_upload_i64(cc, vp, C.size_t(len(vals)), &h) })
		defer C.ps_scalars_free(h)
		devs[d] = hm.dev[d]
		devs[d].sol = h
	}
	A, B, Cc := make([]byte, g1Wire), make([]byte, g2Wire), make([]byte, g1Wire)
	check(func() C.int {
		return C.ps_groth16_prove_multi(cdev, C.size_t(len(hm.dev)), u8(rb), u8(sb), u8(A), u8(B), u8(Cc))
	})
	return Groth16Proof{
		tp: groth16ToxicProof{R: r, S: s},
		A:  pointFrom(C.PS_G1, A, zeroG1),
		B:  pointFrom(C.PS_G2, B, zeroG2),
		C:  pointFrom(C.PS_G1, Cc, zeroG1),
	}
}

// ---------------------------------------------------------------------------------------
// PHGR13 / Pinocchio (pinochio.go)
// ---------------------------------------------------------------------------------------

type HipPHGR13 struct {
	ek     C.ps_phgr13_ek
	vk     C.ps_phgr13_vk
	arrays []*C.ps_points
	qap    *HipQAP
}

func NewHipPHGR13(setup PHGR13Setup, q *HipQAP) *HipPHGR13 {
	hp := &HipPHGR13{qap: q}
	up := func(group C.int, pts []Commit) *C.ps_points {
		h := uploadPoints(group, pts)
		hp.arrays = append(hp.arrays, h)
		return h
	}
	ek := setup.EK
	hp.ek.vs, hp.ek.ws, hp.ek.ys = up(C.PS_G1, ek.vs), up(C.PS_G2, ek.ws), up(C.PS_G1, ek.ys)
	hp.ek.vas, hp.ek.was, hp.ek.yas = up(C.PS_G1, ek.vas), up(C.PS_G1, ek.was), up(C.PS_G1, ek.yas)
	hp.ek.gsi = up(C.PS_G1, ek.gsi)
	// wbs is declared []G2 (pinochio.go:60) but generated from g1w: G1 points (pinochio.go:136)
	hp.ek.vbs, hp.ek.wbs, hp.ek.ybs = up(C.PS_G1, ek.vbs), up(C.PS_G1, ek.wbs), up(C.PS_G1, ek.ybs)
	vk := setup.VK
	diff := q.nbVars - q.nbIO // the reference's split (pinochio.go:291)
	hp.vk.vs_io, hp.vk.ws_io, hp.vk.ys_io = up(C.PS_G1, vk.vs[:diff]), up(C.PS_G2, vk.ws[:diff]), up(C.PS_G1, vk.ys[:diff])
	copyTo(unsafe.Pointer(&hp.vk.av[0]), affineOf(C.PS_G2, vk.av))
	copyTo(unsafe.Pointer(&hp.vk.aw[0]), affineOf(C.PS_G1, vk.aw)) // declared G2, a G1 element (pinochio.go:146)
	copyTo(unsafe.Pointer(&hp.vk.ay[0]), affineOf(C.PS_G2, vk.ay))
	copyTo(unsafe.Pointer(&hp.vk.gamma[0]), affineOf(C.PS_G2, vk.gamma))
	copyTo(unsafe.Pointer(&hp.vk.bgamma[0]), affineOf(C.PS_G1, vk.bgamma))
	copyTo(unsafe.Pointer(&hp.vk.bgamma2[0]), affineOf(C.PS_G2, vk.bgamma2))
	copyTo(unsafe.Pointer(&hp.vk.yts[0]), affineOf(C.PS_G2, vk.yts))
	return hp
}

func (hp *HipPHGR13) Free() {
	for _, p := range hp.arrays {
		C.ps_points_free(p)
	}
}

func bytesOf(p unsafe.Pointer, n int) []byte { return C.GoBytes(p, C.int(n)) }

// PHGR13ProveHIP replaces `func PHGR13Prove(ek PHGR13EvalKey, qap QAP, solution Vector) PHGR13Proof`
// (pinochio.go:207-254).  Deterministic.
func PHGR13ProveHIP(hp *HipPHGR13, solution Vector) PHGR13Proof {
	dsol := uploadSolution(solution)
	defer C.ps_scalars_free(dsol)
	var out C.ps_phgr13_proof
	call(func() C.int { return C.ps_phgr13_prove(hipCtx, &hp.ek, hp.qap.h, dsol, &out) })
	g1 := func(p *C.uint8_t) Commit { return pointFrom(C.PS_G1, bytesOf(unsafe.Pointer(p), g1Wire), zeroG1) }
	return PHGR13Proof{
		vss:  g1(&out.vss[0]),
		vass: g1(&out.vass[0]),
		wss:  pointFrom(C.PS_G2, bytesOf(unsafe.Pointer(&out.wss[0]), g2Wire), zeroG2),
		wass: g1(&out.wass[0]),
		yss:  g1(&out.yss[0]),
		yass: g1(&out.yass[0]),
		hs:   g1(&out.hs[0]),
		gz:   g1(&out.gz[0]),
	}
}

// ToLagrange adds gsi's Lagrange form on the nodes n+1..2n-1 to the key (ps_phgr13_ek.lgsi), computed on the GPU from gsi
// alone (ps_points_monomial_to_lagrange, once per key): hs is then a sum over the values of h, without interpolating it.
// The proof bytes do not change.
func (hp *HipPHGR13) ToLagrange() {
	if hp.ek.lgsi != nil {
		return
	}
	var lgsi *C.ps_points
	call(func() C.int { return C.ps_points_monomial_to_lagrange(hipCtx, hp.qap.h, hp.ek.gsi, 1, &lgsi) })
	hp.arrays = append(hp.arrays, lgsi)
	hp.ek.lgsi = lgsi
}

// PHGR13ProveHIPBatch is PHGR13ProveHIP for many witnesses of ONE circuit under one key, in one call
// (ps_phgr13_prove_batch): one pass of wire values and gate checks over all witnesses, the h sums as one batched sum and
// the other seven elements of all proofs as one batched sum over seven arrays with one digit sort.  The route needs lgsi,
// so a key that came from the reference's setup is converted first (ToLagrange, once per key).  Proof j is the proof
// PHGR13ProveHIP makes of sols[j].  A witness that violates a gate panics with the reference's "apocalypse"
// (qap.go:158-160).
func PHGR13ProveHIPBatch(hp *HipPHGR13, sols []Vector) []PHGR13Proof {
	k := len(sols)
	if k == 0 {
		return nil
	}
	hp.ToLagrange()
	flat := make(Vector, 0, k*len(sols[0]))
	for _, s := range sols {
		if len(s) != len(sols[0]) {
			panic("PHGR13ProveHIPBatch: the witnesses of one circuit have one length")
		}
		flat = append(flat, s...)
	}
	dsols := uploadSolution(flat)
	defer C.ps_scalars_free(dsols)
	raw := make([]C.ps_phgr13_proof, k)
	call(func() C.int { return C.ps_phgr13_prove_batch(hipCtx, &hp.ek, hp.qap.h, dsols, C.size_t(k), &raw[0], nil) })
	g1 := func(p *C.uint8_t) Commit { return pointFrom(C.PS_G1, bytesOf(unsafe.Pointer(p), g1Wire), zeroG1) }
	out := make([]PHGR13Proof, k)
	for j := range out {
		o := &raw[j]
		out[j] = PHGR13Proof{
			vss:  g1(&o.vss[0]),
			vass: g1(&o.vass[0]),
			wss:  pointFrom(C.PS_G2, bytesOf(unsafe.Pointer(&o.wss[0]), g2Wire), zeroG2),
			wass: g1(&o.wass[0]),
			yss:  g1(&o.yss[0]),
			yass: g1(&o.yass[0]),
			hs:   g1(&o.hs[0]),
			gz:   g1(&o.gz[0]),
		}
	}
	return out
}

// PHGR13VerifyHIP replaces `func PHGR13Verify(vk PHGR13VerifKey, qap QAP, p PHGR13Proof, io Vector) bool`
// (pinochio.go:281-378).
func PHGR13VerifyHIP(hp *HipPHGR13, p PHGR13Proof, io Vector) bool {
	var in C.ps_phgr13_proof
	copyTo(unsafe.Pointer(&in.vss[0]), affineOf(C.PS_G1, p.vss))
	copyTo(unsafe.Pointer(&in.vass[0]), affineOf(C.PS_G1, p.vass))
	copyTo(unsafe.Pointer(&in.wss[0]), affineOf(C.PS_G2, p.wss))
	copyTo(unsafe.Pointer(&in.wass[0]), affineOf(C.PS_G1, p.wass))
	copyTo(unsafe.Pointer(&in.yss[0]), affineOf(C.PS_G1, p.yss))
	copyTo(unsafe.Pointer(&in.yass[0]), affineOf(C.PS_G1, p.yass))
	copyTo(unsafe.Pointer(&in.hs[0]), affineOf(C.PS_G1, p.hs))
	copyTo(unsafe.Pointer(&in.gz[0]), affineOf(C.PS_G1, p.gz))
	dio := uploadSolution(io)
	defer C.ps_scalars_free(dio)
	var ok C.int
	call(func() C.int { return C.ps_phgr13_verify(hipCtx, &hp.vk, dio, &in, &ok) })
	return ok != 0
}

// PHGR13VerifyBatchHIP checks many proofs under one key in one call (ps_phgr13_verify_batch): the five pairing products of
// PHGR13Verify (pinochio.go:281-378), each weighted by a random linear combination over the proofs and each with its own
// final exponentiation.  The weights are drawn here, after the proofs are in hand, 128 bits each.  The second result is
// the mask of the equations that did not hold (bit 0 division, 1 v, 2 w, 3 y, 4 linear), 0 for an accepted batch.
func PHGR13VerifyBatchHIP(hp *HipPHGR13, proofs []PHGR13Proof, ios []Vector) (bool, uint32) {
	if len(proofs) != len(ios) {
		panic("PHGR13VerifyBatchHIP: one public-input vector per proof")
	}
	if len(proofs) == 0 {
		return true, 0
	}
	raw, rho, all := phgr13BatchInputs(proofs, ios)
	dio := uploadSolution(all)
	defer C.ps_scalars_free(dio)
	var ok C.int
	call(func() C.int {
		return C.ps_phgr13_verify_batch(hipCtx, &hp.vk, dio, &raw[0], C.size_t(len(proofs)), u8(rho), &ok)
	})
	var info C.ps_phgr13_batch_info
	call(func() C.int { return C.ps_phgr13_verify_batch_info(hipCtx, &info) })
	return ok != 0, uint32(info.failed)
}

// phgr13BatchInputs lays the proofs out as the batch entries take them, draws one 128-bit weight per proof (after the proofs
// are in hand) and joins the public inputs proof-major.
func phgr13BatchInputs(proofs []PHGR13Proof, ios []Vector) ([]C.ps_phgr13_proof, []byte, Vector) {
	var all Vector
	raw := make([]C.ps_phgr13_proof, len(proofs))
	rho := make([]byte, 32*len(proofs))
	for i, p := range proofs {
		all = append(all, ios[i]...)
		in := &raw[i]
		copyTo(unsafe.Pointer(&in.vss[0]), affineOf(C.PS_G1, p.vss))
		copyTo(unsafe.Pointer(&in.vass[0]), affineOf(C.PS_G1, p.vass))
		copyTo(unsafe.Pointer(&in.wss[0]), affineOf(C.PS_G2, p.wss))
		copyTo(unsafe.Pointer(&in.wass[0]), affineOf(C.PS_G1, p.wass))
		copyTo(unsafe.Pointer(&in.yss[0]), affineOf(C.PS_G1, p.yss))
		copyTo(unsafe.Pointer(&in.yass[0]), affineOf(C.PS_G1, p.yass))
		copyTo(unsafe.Pointer(&in.hs[0]), affineOf(C.PS_G1, p.hs))
		copyTo(unsafe.Pointer(&in.gz[0]), affineOf(C.PS_G1, p.gz))
		for zero := true; zero; { // 128 random bits, drawn again in the (2^-128) case that they are all zero
			random.Bytes(rho[32*i+16:32*i+32], random.New())
			for _, b := range rho[32*i+16 : 32*i+32] {
				zero = zero && b == 0
			}
		}
	}
	return raw, rho, all
}

// PHGR13VerifyBatchLocateHIP names the invalid proofs of a batch and the equations each one violates
// (ps_phgr13_verify_batch_locate): the batch check of PHGR13VerifyBatchHIP first, then, if it fails, a bisection over partial
// results kept on the device, every half tested only on the equations its parent failed -- at most 1 + 2 b ceil(log2 N)
// checks for b invalid proofs among N.  The weights are drawn here, as in PHGR13VerifyBatchHIP.  Returns the indices of the
// invalid proofs in ascending order (nil for an accepted batch), their masks (bit 0 division, 1 v, 2 w, 3 y, 4 linear) in the
// same order, and the number of pairing products evaluated.
func PHGR13VerifyBatchLocateHIP(hp *HipPHGR13, proofs []PHGR13Proof, ios []Vector) ([]int, []uint8, int) {
	if len(proofs) != len(ios) {
		panic("PHGR13VerifyBatchLocateHIP: one public-input vector per proof")
	}
	if len(proofs) == 0 {
		return nil, nil, 0
	}
	raw, rho, all := phgr13BatchInputs(proofs, ios)
	dio := uploadSolution(all)
	defer C.ps_scalars_free(dio)
	valid := make([]byte, len(proofs))
	failed := make([]byte, len(proofs))
	var ninvalid C.size_t
	var info C.ps_phgr13_locate_info
	call(func() C.int {
		return C.ps_phgr13_verify_batch_locate(hipCtx, &hp.vk, dio, &raw[0], C.size_t(len(proofs)), u8(rho), u8(valid), u8(failed), &ninvalid)
	})
	call(func() C.int { return C.ps_phgr13_verify_batch_locate_info(hipCtx, &info) })
	var bad []int
	var masks []uint8
	for i, v := range valid {
		if v == 0 {
			bad = append(bad, i)
			masks = append(masks, failed[i])
		}
	}
	return bad, masks, int(info.products)
}

// HipPHGR13Multi: every device holds only ITS index ranges of the evaluation key -- vs .. ybs over len(vs), gsi over
// n-1 -- its own QAP of the circuit and its own copy of the solution.  The quotient runs once, on device 0; the other
// devices copy their range of h from it device to device.
type HipPHGR13Multi struct {
	hd     *HipDevices
	dev    []C.ps_phgr13_device
	qaps   []*C.ps_qap
	arrays []*HipShardedPoints
}

func NewHipPHGR13Multi(hd *HipDevices, ek PHGR13EvalKey, circuit R1CS) *HipPHGR13Multi {
	hm := &HipPHGR13Multi{hd: hd, dev: make([]C.ps_phgr13_device, len(hd.ctxs))} // zero-initialised, as the header requires (lgsi NULL)
	up := func(group C.int, pts []Commit) *HipShardedPoints {
		sp := hd.UploadPoints(group, pts)
		hm.arrays = append(hm.arrays, sp)
		return sp
	}
	// check() panics on a library error: a device that fails after others succeeded must not leak their QAPs and shards
	done := false
	defer func() {
		if !done {
			hm.Free()
		}
	}()
	vs, ws, ys := up(C.PS_G1, ek.vs), up(C.PS_G2, ek.ws), up(C.PS_G1, ek.ys)
	vas, was, yas := up(C.PS_G1, ek.vas), up(C.PS_G1, ek.was), up(C.PS_G1, ek.yas)
	gsi := up(C.PS_G1, ek.gsi)
	// wbs is declared []G2 (pinochio.go:60) but generated from g1w: G1 points (pinochio.go:136)
	vbs, wbs, ybs := up(C.PS_G1, ek.vbs), up(C.PS_G1, ek.wbs), up(C.PS_G1, ek.ybs)
	l, r, o := newCsr(circuit.left), newCsr(circuit.right), newCsr(circuit.out)
	defer l.free()
	defer r.free()
	defer o.free()
	for d, c := range hd.ctxs {
		var q *C.ps_qap
		cc := c
		check(func() C.int {
			return C.ps_qap_create(cc, C.size_t(len(circuit.left)), C.size_t(len(circuit.vars)), C.size_t(circuit.nbIO()), &l.csr, &r.csr, &o.csr, &q)
		})
		hm.qaps = append(hm.qaps, q)
		hm.dev[d].ctx, hm.dev[d].qap = c, q
		e := &hm.dev[d].ek
		e.vs, e.ws, e.ys = vs.parts[d], ws.parts[d], ys.parts[d]
		e.vas, e.was, e.yas = vas.parts[d], was.parts[d], yas.parts[d]
		e.gsi = gsi.parts[d]
		e.vbs, e.wbs, e.ybs = vbs.parts[d], wbs.parts[d], ybs.parts[d]
	}
	done = true
	return hm
}

func (hm *HipPHGR13Multi) Free() {
	for _, q := range hm.qaps {
		C.ps_qap_free(q)
	}
	for _, a := range hm.arrays {
		a.Free()
	}
}

// PHGR13ProveHIPMulti is PHGR13Prove (pinochio.go:207-254) over the devices of this process: same proof bytes as
// PHGR13ProveHIP.  Deterministic.
func PHGR13ProveHIPMulti(hm *HipPHGR13Multi, sol Vector) PHGR13Proof {
	hm.hd.mu.Lock()
	defer hm.hd.mu.Unlock()
	vals := make([]C.int64_t, len(sol))
	for i, v := range sol {
		vals[i] = C.int64_t(v)
	}
	// the device structs go to C memory: they hold C pointers only, but live in a Go slice
	cdev := (*C.ps_phgr13_device)(C.malloc(C.size_t(len(hm.dev)) * C.size_t(unsafe.Sizeof(hm.dev[0]))))
	defer C.free(unsafe.Pointer(cdev))
	devs := (*[1 << 16]C.ps_phgr13_device)(unsafe.Pointer(cdev))[:len(hm.dev):len(hm.dev)]
	var vp *C.int64_t // an empty solution has no first element to point at (the library refuses it by length, not by a Go panic here)
	if len(vals) > 0 {
		vp = &vals[0]
	}
	for d := range hm.dev {
		var h *C.ps_scalars
		cc := hm.dev[d].ctx
		check(func() C.int { return C.ps_scalars_upload_i64(cc, vp, C.size_t(len(vals)), &h) })
		defer C.ps_scalars_free(h)
		devs[d] = hm.dev[d]
		devs[d].sol = h
	}
	var out C.ps_phgr13_proof
	check(func() C.int { return C.ps_phgr13_prove_multi(cdev, C.size_t(len(hm.dev)), &out) })
	g1 := func(p *C.uint8_t) Commit { return pointFrom(C.PS_G1, bytesOf(unsafe.Pointer(p), g1Wire), zeroG1) }
	return PHGR13Proof{
		vss:  g1(&out.vss[0]),
		vass: g1(&out.vass[0]),
		wss:  pointFrom(C.PS_G2, bytesOf(unsafe.Pointer(&out.wss[0]), g2Wire), zeroG2),
		wass: g1(&out.wass[0]),
		yss:  g1(&out.yss[0]),
		yass: g1(&out.yass[0]),
		hs:   g1(&out.hs[0]),
		gz:   g1(&out.gz[0]),
	}
}

// ---------------------------------------------------------------------------------------
// the reference's own tests, pointed at the GPU backend (groth16_test.go:22-30, pinocchio_test.go:23-29):
//
//	r1cs := createR1CS(); s := createWitness(r1cs); qap := ToQAP(r1cs)
//	hq := NewHipQAP(r1cs)
//	tr := NewGroth16TrustedSetup(qap); hs := NewHipGroth16(tr, hq)
//	proof := Groth16ProveHIP(hs, s)
//	require.True(t, Groth16Verify(tr, qap, proof, s[:qap.nbVars-qap.nbIO]))     // the reference's CPU verifier
//	require.True(t, Groth16VerifyHIP(hs, proof, s[:qap.nbVars-qap.nbIO]))      // or the library's
//	setup := NewPHGR13TrustedSetup(qap); hp := NewHipPHGR13(setup, hq)
//	require.True(t, PHGR13Verify(setup.VK, qap, PHGR13ProveHIP(hp, s), s[:qap.nbVars-qap.nbIO]))
//	require.True(t, hq.IsValidHIP(s))                                            // TestQAPValidity, qap_test.go
//	hd := NewHipDevices(8); hm := NewHipGroth16Multi(hd, tr, r1cs)              // one process, eight GPUs
//	require.True(t, Groth16Verify(tr, qap, Groth16ProveHIPMulti(hm, s), s[:qap.nbVars-qap.nbIO]))
//	hpm := NewHipPHGR13Multi(hd, setup.EK, r1cs)                                 // PHGR13 on the same eight GPUs
//	require.True(t, PHGR13Verify(setup.VK, qap, PHGR13ProveHIPMulti(hpm, s), s[:qap.nbVars-qap.nbIO]))
// ---------------------------------------------------------------------------------------
