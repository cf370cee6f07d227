/*
 * druggen_hip_desc.h -- the descriptor entry of libdruggen_hip.so (gfx950 / MI355X): rotatable bonds, a topological polar
 * surface area from a host-made table, ring and carbon counts, and a per-atom environment key, of molecules that
 * dg_mol_validity (druggen_hip_valid.h) found valid.  Same conventions as druggen_hip.h (device pointers, the caller's stream,
 * 0 / DG_E_* / hipError_t return values, dg_last_error_string()).  A fifth header because the first four are pinned, prototype
 * by prototype, to DG_VERSION 232 and their ctypes tables (druggen_amd/_lib.py SIGNATURES / TEXT_SIGNATURES / FP_SIGNATURES /
 * VALID_SIGNATURES); the entry here is typed from DESC_SIGNATURES of the same file and checked the same way
 * (tests/test_mol_desc_host.py).
 */
#ifndef DRUGGEN_HIP_DESC_H
#define DRUGGEN_HIP_DESC_H

#include "druggen_hip_valid.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- descriptors of valid molecules (csrc/mol_desc.hip) ---- */
#define DG_DESC_FIELDS         12            /* int32 entries of a row of `desc` */
#define DG_DESC_MAX_ENV        4096          /* the most rows of env_table */
#define DG_DESC_NO_KEY         0xFFFFFFFFu   /* atom_key outside the scope, and everywhere unless the status is 0 */
#define DG_DESC_BOND           1             /* bond_class bit 0: a BOND of the scope */
#define DG_DESC_RING_BOND      2             /* bond_class bit 1: a BOND that is no bridge */
#define DG_DESC_ROTATABLE      4             /* bond_class bit 2: a rotatable BOND */

/* dg_mol_descriptors: per molecule of a batch that dg_mol_validity has checked, the counts that drug-likeness rules are made of.
 * One workgroup per molecule, the graph in LDS; integers only, no atomics on global memory, no host synchronisation
 * (capturable), nothing allocated.  This is the project's own, exactly specified definition: NOT RDKit's
 * CalcNumRotatableBonds (the rotatable bonds here are the SIMPLE pattern -- a single bond outside every ring between two atoms
 * that each have another neighbour, no triple bond at either end -- not RDKit's strict one, which also drops amides, esters and
 * the like), NOT RDKit's CalcTPSA (the values come from the caller's table; the built-in one of druggen_amd/descriptors.py has
 * N and O rows only, no S or P contributions), and no logP.
 *
 * The graph: atoms [B,N] u8 labels, bonds [B,cap,4] u8 rows (hi, lo, label, 0) (4-byte aligned), n_bonds [B] -- as
 * dg_decode_graph wrote them.  `scope` selects the atoms: DG_CANON_LARGEST those with component[b,i] == largest[b];
 * DG_CANON_WHOLE every atom except isolated pads (label 0 and no bond row).  component / largest are read under
 * DG_CANON_LARGEST only.  Only the first min(n_bonds, cap) rows are read, and only rows with both ends in the scope count:
 * these are the BONDS below (rows with hi == lo or an end >= N are skipped; the decode lists none, and no pair twice -- a
 * list that names a pair twice is outside this definition).  flags [B] (may be NULL): a negative value means the molecule
 * has no graph; so does n_bonds > cap.  This is the scope rule and the BONDS of dg_mol_validity and dg_mol_fingerprint.
 *
 * From dg_mol_validity of the SAME batch under the SAME scope: mol [B,DG_VALID_MOL_FIELDS] i32, of which only the status
 * (entry 0) is read, and hcount [B,N] u8.  A record of another batch or scope is outside this definition (the kernel stays
 * inside its arrays whatever it holds).
 *
 * The tables (device memory, made by the host; the kernel knows no chemistry):
 *   bond_table [n_bond_labels] u32: order | aromatic << 8, the table of dg_mol_validity.
 *   atom_flags [n_atom_labels] u32: the flags column of dg_mol_validity's atom_table; bit 0: a polar atom.
 *   atom_class [n_atom_labels] u32: bit 0: a carbon.
 *   env_table  [n_env,4] u32: rows (key, tpsa in 1e-2 A^2, 0, 0), keys STRICTLY ASCENDING, 0 <= n_env <= DG_DESC_MAX_ENV.  The
 *     kernel does not check the order: an unsorted table is the host's error (druggen_amd/descriptors.py refuses it).
 *
 * status[b]: DG_VALID_NO_GRAPH if the list is truncated (n_bonds > cap) or flags < 0, else mol[b,0].
 *
 * Definition, for a molecule of status 0, per atom a of the scope ("bonds of a": the BONDS with a as one end):
 *   n1[a], n2[a], n3[a]  its bonds of table order 1 that are not aromatic, of order 2, of order 3;
 *   na[a]                its aromatic bonds;           deg[a] = n1 + n2 + n3 + na;          h[a] = hcount[b,a];
 *   r3[a]                1 iff two neighbours of a are bonded to each other (a lies in a triangle of BONDS), else 0;
 *   key[a] = label | h << 8 | n1 << 12 | n2 << 16 | n3 << 19 | na << 21 | r3 << 24.
 * The fields fit, from the valence bound of 8 of dg_mol_validity (w0[a] <= 8): h + n1 + 2 n2 + 3 n3 + na <= w0[a] <= 8, so
 * label <= 254 (8 bits), h <= 8 and n1 <= 8 (4 bits each), n2 <= 4 (3 bits), n3 <= 2 (2 bits) and na <= 8.  na has 3 bits: na
 * <= 7 fits, and na == 8 forces h = n1 = n2 = n3 = 0 and carries into bit 24, where the key reads (label, na = 0, r3 = 1, all
 * else 0); no other atom has that key, because r3 = 1 needs two neighbours and so a non-zero n1, n2, n3 or na field.  Equal
 * keys mean equal (label, h, n1, n2, n3, na, r3) -- except that an atom with eight aromatic bonds loses its r3 bit, which
 * then reads 1 -- and bits 25..31 are zero.
 *   A BOND is a RING BOND iff it is not a bridge: its ends stay connected without it (the ring notion of druggen_hip_fp.h and
 *     druggen_hip_valid.h).
 *   A BOND is ROTATABLE iff it has table order 1, is not aromatic, is a bridge, both ends have deg >= 2 and n3 == 0.
 *   tpsa[a] = the value of the env_table row whose key equals key[a]; 0 if there is none.  a is UNTYPED iff it is polar
 *     (atom_flags bit 0 of its label) and no row has its key.
 *
 * Outputs, every element stored by every call (but the bond_class entries past min(n_bonds, cap)):
 *   desc [B,12] i32: status; and for status 0 -- all of them 0 otherwise --
 *       n_heavy           the atoms of the scope;
 *       n_rot             the rotatable BONDS;
 *       tpsa              the sum of tpsa[a] over the scope, in 1e-2 A^2, modulo 2^32;
 *       n_untyped         the untyped atoms;
 *       n_rings           BONDS - n_heavy + the connected components of the scope (the cyclomatic number);
 *       n_ring_atoms      the atoms with a ring bond;
 *       n_aromatic_atoms  the atoms with na > 0;
 *       n_carbon          the atoms whose label is a carbon (atom_class bit 0);
 *       n_sp3_carbon      the carbons with n2 = n3 = na = 0;
 *     then two reserved entries, 0.
 *   atom_key [B,N] u32: key[a] for the atoms of the scope of a molecule of status 0; DG_DESC_NO_KEY outside the scope and
 *     everywhere for any other status.
 *   bond_class [B,cap] u8: for the first min(n_bonds, cap) rows of the bond list, DG_DESC_BOND | DG_DESC_RING_BOND |
 *     DG_DESC_ROTATABLE as they apply; 0 for a row that is no BOND and for every row when status != 0.  The entries past
 *     min(n_bonds, cap) are not touched.
 * All outputs are functions of the input alone: pinned values, no certificate.
 *
 * B < 0, N outside 1..256, cap < 0, n_atom_labels outside 1..255, n_bond_labels outside 1..256 or n_env outside
 * 0..DG_DESC_MAX_ENV: DG_E_SHAPE; a scope other than 0 / 1, a null pointer (bonds and bond_class may be NULL when cap == 0,
 * component / largest unless scope == 1, env_table when n_env == 0, flags always) or a misaligned one (bonds, the tables, the
 * int arrays, desc and atom_key: 4 bytes): DG_E_ARG.  The shape is checked first, then the scope.  B == 0 returns 0 without a
 * launch.  No bond count up to cap and no N up to 256 is refused: the bond list is read from global memory. */
int dg_mol_descriptors(const unsigned char* atoms, const unsigned char* bonds, const int* n_bonds, const unsigned char* component,
                       const int* largest, const int* flags, const int* mol, const unsigned char* hcount,
                       const unsigned* bond_table, int n_bond_labels, const unsigned* atom_flags, const unsigned* atom_class,
                       int n_atom_labels, const unsigned* env_table, int n_env, int B, int N, int cap, int scope, int* desc,
                       unsigned* atom_key, unsigned char* bond_class, dg_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* DRUGGEN_HIP_DESC_H */
