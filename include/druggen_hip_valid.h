/*
 * druggen_hip_valid.h -- the validity entry of libdruggen_hip.so (gfx950 / MI355X): is a decoded graph a molecule -- allowed
 * valences, aromatic bonds in rings, a Kekule structure -- and, if so, its hydrogens, mass and polar atoms.  Same conventions as
 * druggen_hip.h (device pointers, the caller's stream, 0 / DG_E_* / hipError_t return values, dg_last_error_string()).  A fourth
 * header because the first three are pinned, prototype by prototype, to DG_VERSION 232 and their ctypes tables
 * (druggen_amd/_lib.py SIGNATURES / TEXT_SIGNATURES / FP_SIGNATURES); the entry here is typed from VALID_SIGNATURES of the same
 * file and checked the same way (tests/test_mol_valid_host.py).
 */
#ifndef DRUGGEN_HIP_VALID_H
#define DRUGGEN_HIP_VALID_H

#include "druggen_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- validity of decoded molecules (csrc/mol_valid.hip) ---- */
#define DG_VALID_OK                   0      /* status: none of the below */
#define DG_VALID_NO_GRAPH             (-2)   /* the bond list was truncated (n_bonds > cap) or flags < 0 */
#define DG_VALID_EMPTY                1      /* the scope has no atom */
#define DG_VALID_UNKNOWN_LABEL        2      /* an atom of the scope or a BOND has an unknown label */
#define DG_VALID_OVER_VALENT          3      /* some atom has no allowed valence >= sigma */
#define DG_VALID_AROMATIC_NOT_IN_RING 4      /* some aromatic BOND is a bridge */
#define DG_VALID_NOT_KEKULISABLE      5      /* the aromatic graph G has no perfect matching */
#define DG_VALID_MOL_FIELDS           8      /* int32 entries of a row of `mol` */

/* dg_mol_validity: per molecule of a batch, a status, the implicit hydrogens of every atom, the mass and the polar atoms, and
 * a Kekule structure as a certificate.  One workgroup per molecule; integers only, no atomics on global memory, no host
 * synchronisation (capturable), nothing allocated.  This is the project's own, exactly specified check, NOT RDKit's
 * SanitizeMol: no charges, radicals or explicit hydrogens, no aromaticity perception, no ring-size or Hueckel rule.
 *
 * The graph: atoms [B,N] u8 labels, bonds [B,cap,4] u8 rows (hi, lo, label, 0) (4-byte aligned), n_bonds [B] -- as
 * dg_decode_graph wrote them.  `scope` selects the atoms: DG_CANON_LARGEST those with component[b,i] == largest[b];
 * DG_CANON_WHOLE every atom except isolated pads (label 0 and no bond row).  component / largest are read under
 * DG_CANON_LARGEST only.  Only the first min(n_bonds, cap) rows are read, and only rows with both ends in the scope count:
 * these are the BONDS below (rows with hi == lo or an end >= N are skipped; the decode lists none, and no pair twice -- a
 * list that names a pair twice is outside this definition).  flags [B] (may be NULL): a negative value means the molecule
 * has no graph; so does n_bonds > cap.  This is the scope rule and the BONDS of dg_mol_fingerprint (druggen_hip_fp.h).
 *
 * The tables (device memory, made by the host; the kernel knows no chemistry):
 *   atom_table [n_atom_labels,4] u32: (valences, mass, flags, 0) per atom label.  valences: four bytes, byte k in bits
 *     8 k .. 8 k + 7; the allowed valences are the bytes before the first zero byte (the host lists them ascending).  mass in
 *     1e-4 Da.  flags bit 0: a polar atom.  The row is UNKNOWN if byte 0 is zero or any of the four bytes exceeds 8.
 *   bond_table [n_bond_labels] u32: order | aromatic << 8.  The row is UNKNOWN if order is 0 or above 3, if aromatic is set
 *     and order is not 1, or if a bit above bit 8 is set.
 * A label without a table row is UNKNOWN.
 *
 * Definition, per atom a of the scope ("bonds of a": the BONDS with a as one end):
 *   sigma[a]  the sum of `order` over the bonds of a (an aromatic bond counts 1);
 *   arom[a]   the number of aromatic bonds of a;
 *   w0[a]     the smallest allowed valence >= sigma[a]; a is OVER-VALENT if there is none;
 *   a is a CANDIDATE iff arom[a] > 0 and w0[a] > sigma[a]: it can take the double bond of a Kekule structure.
 * The aromatic graph G: the candidates as vertices, the aromatic bonds with both ends candidates as edges (degree <= 7, since
 * arom[a] <= sigma[a] < w0[a] <= 8).  A bond is a BRIDGE if its ends are not connected without it -- it lies on no cycle of the
 * graph of the BONDS, the ring notion of druggen_hip_fp.h.
 *
 * status, the first of these that applies:
 *   DG_VALID_NO_GRAPH (-2)             the list is truncated or flags < 0;
 *   DG_VALID_EMPTY (1)                 the scope has no atom;
 *   DG_VALID_UNKNOWN_LABEL (2)         an atom of the scope or a BOND has an UNKNOWN label;
 *   DG_VALID_OVER_VALENT (3)           some atom of the scope is over-valent;
 *   DG_VALID_AROMATIC_NOT_IN_RING (4)  some aromatic BOND is a bridge;
 *   DG_VALID_NOT_KEKULISABLE (5)       G has no perfect matching;
 *   DG_VALID_OK (0)                    none of the above.
 * The matching is computed for status 5 and 0 only (a maximum matching of a general graph: Edmonds' blossom algorithm).
 *
 * Outputs, every element stored by every call (but the rows of kekule past min(n_bonds, cap)):
 *   mol [B,8] i32: status; n_atoms, the atoms of the scope (0 for status -2); n_over, the over-valent atoms (0 for status -2,
 *     1, 2); deficiency, the candidates that a MAXIMUM matching of G leaves unmatched (0 iff G has a perfect matching; -1 when
 *     the matching was not computed, status -2 and 1..4); and, for status 0 -- all four are 0 otherwise --
 *       n_h          the sum over the scope of h[a] = w0[a] - sigma[a] - (1 if a is a candidate, else 0);
 *       mass         the sum over the scope of the atoms' masses, plus n_h * h_mass, modulo 2^32;
 *       n_donors     the polar atoms with h[a] >= 1;
 *       n_acceptors  the polar atoms.
 *   hcount [B,N] u8: h[a] for the atoms of the scope of a molecule of status 0; 0xFF outside the scope and everywhere for any
 *     other status.
 *   kekule [B,cap,4] u8: the first min(n_bonds, cap) rows are (hi, lo, label, order) of the input row with a Kekule order:
 *     for status 0 and a BOND, the table's order 1 / 2 / 3, an aromatic bond 2 if it is in the matching and 1 if not; 0 for a
 *     row that is no BOND and for every row when status != 0.  The rows past min(n_bonds, cap) are not touched.
 * mol and hcount are functions of the input alone.  kekule depends on which perfect matching was found: it is a certificate
 * -- every candidate has exactly one aromatic bond of order 2, no other atom has one, and the orders at a plus h[a] give
 * w0[a] -- and the same bytes on every run of the same input, but no pinned value.
 *
 * B < 0, N outside 1..256, cap < 0, n_atom_labels outside 1..255 or n_bond_labels outside 1..256: DG_E_SHAPE; a scope other
 * than 0 / 1, h_mass < 0, a null pointer (bonds and kekule may be NULL when cap == 0, component / largest unless scope == 1,
 * flags always) or a misaligned one (bonds, kekule, the tables and the int arrays: 4 bytes): DG_E_ARG.  The shape is checked
 * first, then the scope.  B == 0 returns 0 without a launch.  No bond count up to cap and no N up to 256 is refused: the bond
 * list is read from global memory. */
int dg_mol_validity(const unsigned char* atoms, const unsigned char* bonds, const int* n_bonds, const unsigned char* component,
                    const int* largest, const int* flags, const unsigned* atom_table, int n_atom_labels,
                    const unsigned* bond_table, int n_bond_labels, int B, int N, int cap, int scope, int h_mass, int* mol,
                    unsigned char* hcount, unsigned char* kekule, dg_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* DRUGGEN_HIP_VALID_H */
