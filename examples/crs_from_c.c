/* Minimal C caller of the CRS import (the calls cgo generates for curdlemsm.NewCRS): compiles as strict C99 against
 * include/curdle_msm.h and links with -lcurdlemsm.  Generates a CRS of ell = 8, exports its fields in gnark's layouts,
 * imports them again under CURDLE_CRS_TRUSTED -- the caller made the points itself, so nothing is checked and no GPU is
 * needed -- and compares the wire form of the two handles.
 *
 *   gcc -std=c99 -Iinclude examples/crs_from_c.c -Lgo-curdleproofs_amd -lcurdlemsm \
 *       -Wl,-rpath,$PWD/go-curdleproofs_amd -o /tmp/crs_from_c && /tmp/crs_from_c
 *
 * Exit code 0 = the two handles serialise to the same bytes, 1 = anything else.  A caller whose CRS came from outside
 * passes flags = 0 instead: every point is then checked on the GPU, and a curdle_crs_fault names the first bad one.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "curdle_msm.h"

#define ELL 8

static int fail(const char* what, int rc) {
  char err[256];
  curdle_last_error(err, sizeof(err));
  fprintf(stderr, "%s failed (%d): %s\n", what, rc, err);
  return 1;
}

int main(void) {
  static uint64_t Gs[ELL * CURDLE_G1_AFFINE_U64], Hs[CURDLE_CRS_N_BLINDERS * CURDLE_G1_AFFINE_U64];
  uint64_t H[CURDLE_G1_JAC_U64], Gt[CURDLE_G1_JAC_U64], Gu[CURDLE_G1_JAC_U64];
  uint64_t Gsum[CURDLE_G1_AFFINE_U64], Hsum[CURDLE_G1_AFFINE_U64];
  static uint8_t a[48 * (ELL + 9)], b[48 * (ELL + 9)];
  size_t a_len = 0, b_len = 0;
  curdle_crs_points in;
  curdle_crs_fault fault;
  curdle_crs *generated, *imported = NULL;
  curdle_rand* rand = curdle_rand_new(7);
  int rc;

  if (!rand) return fail("curdle_rand_new", CURDLE_ENOMEM);
  generated = curdle_crs_generate(ELL, rand);
  curdle_rand_free(rand);
  if (!generated) return fail("curdle_crs_generate", CURDLE_ENOMEM);
  rc = curdle_crs_export_points(generated, Gs, Hs, H, Gt, Gu, Gsum, Hsum);
  if (rc != CURDLE_OK) return fail("curdle_crs_export_points", rc);

  in.Gs = Gs;
  in.ell = ELL;
  in.Hs = Hs;
  in.H = H;
  in.Gt = Gt;
  in.Gu = Gu;
  in.Gsum = Gsum;
  in.Hsum = Hsum;
  rc = curdle_crs_from_points(&in, CURDLE_CRS_TRUSTED, &imported, &fault);
  if (rc != CURDLE_OK) return fail("curdle_crs_from_points", rc);
  if (fault.field != -1 || curdle_crs_size(imported) != ELL) return fail("the imported handle", 0);

  rc = curdle_crs_to_bytes(generated, a, sizeof(a), &a_len);
  if (rc != CURDLE_OK) return fail("curdle_crs_to_bytes", rc);
  rc = curdle_crs_to_bytes(imported, b, sizeof(b), &b_len);
  if (rc != CURDLE_OK) return fail("curdle_crs_to_bytes", rc);
  curdle_crs_free(imported);
  curdle_crs_free(generated);
  if (a_len != sizeof(a) || b_len != a_len || memcmp(a, b, a_len) != 0) {
    fprintf(stderr, "the imported CRS serialises differently\n");
    return 1;
  }
  printf("crs ell=%d bytes=%lu first=%02x%02x%02x%02x same=1\n", ELL, (unsigned long)a_len, a[0], a[1], a[2], a[3]);
  return 0;
}
