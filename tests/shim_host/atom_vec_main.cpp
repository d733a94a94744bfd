/* atom_vec_main.cpp -- TEST INFRASTRUCTURE: the program around atom_vec_harness.cpp (oracle/Makefile `ref` builds it into
 * oracle/_ref/atomvec_check and atomvec_check_asan; tests/test_shim_host_paths.py runs them).  Prints "<rc> <message>". */
#include <stdio.h>
extern "C" int atomvec_check(char *, int);
int main() { char m[2048]; int r = atomvec_check(m, 2048); printf("%d %s\n", r, m); return r; }
