// Package curdlecrs hands a curdleproof.CRS to libcurdlemsm.so.  It is a package of its own because curdlemsm cannot
// import the root package: common imports curdlemsm for its MultiExp funnel (INTEGRATION.md section 2) and the root
// package imports common, so a curdlemsm that named curdleproof.CRS would close an import cycle.
//
// UNVERIFIED like everything under go/: there is no Go toolchain in the build image, so this file has never been
// compiled.
package curdlecrs

import (
	curdleproof "github.com/jsign/curdleproofs"
	"github.com/jsign/curdleproofs/curdlemsm"
)

// NewCRS makes a library handle from the Go struct's fields (crs.go:10-18), read in place in gnark's layouts.  Every
// point is checked on the GPU -- range, curve equation, subgroup --, then that no two generators are equal and that
// Gsum and Hsum are the sums of Gs and Hs; a *curdlemsm.CRSFault names the first failure.  The handle opens the
// library's Verify, batch verifiers, Prove, constant-time prover and Whisk shuffle calls to this CRS.
func NewCRS(crs *curdleproof.CRS) (*curdlemsm.CRS, error) {
	return curdlemsm.NewCRSFromFields(crs.Gs, crs.Hs, &crs.H, &crs.Gt, &crs.Gu, &crs.Gsum, &crs.Hsum, false)
}

// NewTrustedCRS is NewCRS for a CRS this process generated itself (GenerateCRS): nothing is checked and no GPU is
// needed.  That every point lies in G1 is then the caller's precondition.
func NewTrustedCRS(crs *curdleproof.CRS) (*curdlemsm.CRS, error) {
	return curdlemsm.NewCRSFromFields(crs.Gs, crs.Hs, &crs.H, &crs.Gt, &crs.Gu, &crs.Gsum, &crs.Hsum, true)
}
