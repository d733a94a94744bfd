/* domain_harness.cpp -- TEST INFRASTRUCTURE (oracle/_ref build only; never shipped, never copied).
 *
 * Driver around the reference's OWN, UNMODIFIED src/domain.cpp, which oracle/Makefile compiles straight from where it
 * lies (with an empty generated style_region.h in front of the include path) and links with this file into the
 * executable oracle/_ref/ref_closest_image.  Domain::closest_image (domain.cpp:1220-1312) is
 * non-virtual and reads only triclinic, {x,y,z}periodic, {x,y,z}prd, {x,y,z}prd_half, xy, xz, yz of its object, so it is
 * called on a zeroed block of memory with those fields set; every other symbol of domain.cpp stays unresolved
 * (-Wl,--unresolved-symbols=ignore-all: an executable, because a shared library would bind the data symbols at load time).
 *
 * This file contains no image arithmetic: every number it writes is computed by the reference's compiled code.
 *
 * Input (file named by argv[1], or stdin), raw native float64:
 *     prd[3]  tilt[3] (xy, xz, yz)  periodic[3]  triclinic  npairs      -- 11 values
 *     npairs x ( xi[3]  xj[3] )
 * Output (stdout), raw float64: npairs x xjimage[3].
 */
#include <cstdio>
#include <cstdlib>
#include <vector>

#include <mpi.h>
#include "domain.h"

using namespace LAMMPS_NS;

int main(int argc, char **argv) {
  FILE *in = argc > 1 ? fopen(argv[1], "rb") : stdin;
  if (!in) { fprintf(stderr, "ref_closest_image: cannot open %s\n", argv[1]); return 2; }
  double head[11];
  if (fread(head, sizeof(double), 11, in) != 11) { fprintf(stderr, "ref_closest_image: short header\n"); return 2; }
  const size_t n = (size_t)head[10];
  std::vector<double> pairs(6 * n), out(3 * n);
  if (fread(pairs.data(), sizeof(double), 6 * n, in) != 6 * n) { fprintf(stderr, "ref_closest_image: short input\n"); return 2; }

  Domain *d = (Domain *)calloc(1, sizeof(Domain) + 64);
  d->xprd = head[0]; d->yprd = head[1]; d->zprd = head[2];
  d->xprd_half = 0.5 * d->xprd; d->yprd_half = 0.5 * d->yprd; d->zprd_half = 0.5 * d->zprd;  /* as set_global_box does, domain.cpp:246-248 */
  d->xy = head[3]; d->xz = head[4]; d->yz = head[5];
  d->xperiodic = (int)head[6]; d->yperiodic = (int)head[7]; d->zperiodic = (int)head[8];
  d->triclinic = (int)head[9];
  for (size_t k = 0; k < n; k++) d->closest_image(&pairs[6 * k], &pairs[6 * k + 3], &out[3 * k]);

  if (fwrite(out.data(), sizeof(double), 3 * n, stdout) != 3 * n) return 3;
  fflush(stdout);
  _Exit(0);   /* no static destructors of the half-linked domain.cpp */
}
