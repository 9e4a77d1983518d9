// Host-only pieces of the principal-coordinates solver (pcoa.hip): the dense symmetric eigensolver of its
// Rayleigh-Ritz step.
#pragma once

// All eigenpairs of the symmetric n x n matrix a (row-major; only its lower triangle is read): Householder
// tridiagonalisation, then implicit QL (EISPACK's tred2 / tql2).  w[n]: the eigenvalues in DESCENDING order; z (n x n):
// ROW j is the unit eigenvector of w[j].  a is destroyed.  O(n^3), no allocation beyond 2 n doubles.
void dvs_symeig_desc(int n, double *a, double *w, double *z);
