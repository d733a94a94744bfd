/* shim_ewald_harness.cpp -- TEST INFRASTRUCTURE (compiled by tests/test_shim_polar_ewald.py where the LAMMPS sources the
 * shim harnesses build against are present).  The recording stub of shim_compute_harness.cpp, with the library's settings
 * saying `polar_ewald`: the reciprocal charge-dipole forces the library adds to atom->f have no f.x virial, so init_style must
 * keep the base class off the fdotr virial and compute() must ask the library for the global virial itself -- with the
 * shim's default half list (device_neigh no, newton_pair on) as well as with the device-built list. */
#include "shim_compute_harness.cpp"

extern "C" int shimewald_check(int *ncombos, char *msg, int nmsg) {
  g_last_error.clear();
  *ncombos = 0;
  const int nlocal = 5, nghost = 3, nall = nlocal + nghost, ntypes = 2;
  World W = make_world(nlocal, nghost, ntypes);
  LAMMPS *lmp = W.lmp; Force *force = W.force; Atom *atom = W.atom; Neighbor *nb = W.nb; NeighList *list = W.list;
  int rc = 0;
  try {
    for (int dn = 0; dn < 2; dn++) {
      memset(&R.st, 0, sizeof(R.st));
      R.st.cut_lj_global = 9.0; R.st.cut_coul = 9.0; R.st.iterations_max = 50; R.st.device_neigh = dn; R.st.polar_ewald = 1e-6;
      R.calls.clear();
      PairLJCutCoulLongPolarizationMI355X *shim = new PairLJCutCoulLongPolarizationMI355X(lmp);
      force->pair = shim;
      shim->ncoultablebits = 0;
      {
        std::string tag = "polar_ewald init, device_neigh " + std::to_string(dn);
        char a0[] = "9.0", a1[] = "9.0"; char *sa[2] = {a0, a1};
        shim->settings(2, sa);
        char c0[] = "*", c1[] = "*", c2[] = "0.1", c3[] = "3.0"; char *ca[4] = {c0, c1, c2, c3};
        shim->coeff(4, ca);
        shim->init_style();
        shim->init_list(0, list);
        EXPECT(shim->no_virial_fdotr_compute == 1, "polar_ewald must keep the base class off the fdotr virial");
      }
      for (int vflag = 0; vflag <= 2; vflag++) {
        std::ostringstream t; t << "polar_ewald device_neigh " << dn << " vflag " << vflag;
        const std::string tag = t.str();
        nb->ago = 0;
        R.rc_compute = POLAR_OK;
        R.calls.clear();
        for (int k = 0; k < 3 * nall; k++) { atom->f[0][k] = 7.0 + 0.5 * k; atom->mu_induced[0][k] = -1.0; atom->ef_static[0][k] = -2.0; }
        for (int k = 0; k < 6; k++) shim->virial[k] = 500.0 + k;
        shim->compute(1, vflag);
        (*ncombos)++;
        const int want_vf = vflag == 0 ? 0 : (dn ? vflag : 1);   /* a global virial request reaches the library, never fdotr */
        EXPECT(R.vflag == want_vf, "vflag handed to the library: " << R.vflag << " expected " << want_vf);
        EXPECT(shim->vflag_fdotr == 0, "the base class must not form sum f.x");
        for (int k = 0; k < 6; k++) {
          const double expect = vflag ? 10.0 + k : 500.0 + k;   /* the library's virial (pair + reciprocal), or untouched */
          EXPECT(shim->virial[k] == expect, "virial[" << k << "] = " << shim->virial[k] << " expected " << expect);
        }
      }
    }
  } catch (Fail &f) {
    snprintf(msg, nmsg, "%s", f.msg.c_str());
    rc = -1;
  } catch (SeamError &e) {
    snprintf(msg, nmsg, "error->all: %s", e.msg.c_str());
    rc = -1;
  }
  return rc;
}
