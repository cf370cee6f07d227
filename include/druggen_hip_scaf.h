/*
 * druggen_hip_scaf.h -- the scaffold entry of libdruggen_hip.so (gfx950 / MI355X): the Murcko-style scaffold of every valid
 * molecule of a batch, written out as a second decoded batch, with ring systems, ring sizes of the ring bonds and atom roles.
 * Same conventions as druggen_hip.h (device pointers, the caller's stream, 0 / DG_E_* / hipError_t return values,
 * dg_last_error_string()).  A seventh header because the first four are pinned, prototype by prototype, to DG_VERSION 232 and
 * the fifth and sixth to their one entry each; the entry here is typed from SCAF_SIGNATURES of druggen_amd/_lib.py and checked
 * the same way (tests/test_mol_scaf_host.py).
 */
#ifndef DRUGGEN_HIP_SCAF_H
#define DRUGGEN_HIP_SCAF_H

#include "druggen_hip_desc.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- scaffolds and ring systems of valid molecules (csrc/mol_scaf.hip) ---- */
#define DG_SCAF_MOL_FIELDS     16            /* int32 entries of a row of `mol` */
#define DG_SCAF_HIST_BINS      8             /* int32 entries of a row of `ring_hist`: sizes 3, 4, 5, 6, 7, 8, 9..12, >= 13 */
#define DG_SCAF_MAX_RING       255           /* the ring size of a ring bond saturates here */
#define DG_SCAF_NO_SYSTEM      255           /* atom_system of an atom without a ring bond */
#define DG_SCAF_ROLE_NONE      0             /* atom_role: outside the scope */
#define DG_SCAF_ROLE_SIDE      1             /* a side-chain atom: in the scope, not in the scaffold */
#define DG_SCAF_ROLE_EXO       2             /* an exo atom */
#define DG_SCAF_ROLE_LINKER    3             /* a core atom without a ring bond */
#define DG_SCAF_ROLE_RING      4             /* an atom with a ring bond */

/* dg_mol_scaffold: per molecule of a batch that dg_mol_descriptors has described, the scaffold -- rings, the linkers between
 * them, and the atoms double-bonded to either -- as the fields of a SECOND decoded batch, so that dg_mol_canon, dg_mol_smiles
 * and every other entry that reads a decoded batch works on scaffolds unchanged; and the ring make-up of the molecule.  One
 * workgroup per molecule, the graph in LDS; integers only, no atomics on global memory, no host synchronisation (capturable),
 * nothing allocated, nothing waits on another workgroup.  This is the project's own, exactly specified definition, written
 * after what RDKit's MurckoScaffold.GetScaffoldForMol is understood to do and NOT checked against it: no smallest set of
 * smallest rings is computed and no ring is enumerated -- the ring sizes are per BOND --, and the scaffold is a labelled
 * graph, not a sanitised canonical SMILES: two Kekule drawings of one scaffold are two scaffolds.
 *
 * The chain is dg_decode_graph -> dg_mol_validity -> dg_mol_descriptors -> dg_mol_scaffold on the SAME batch and cap.
 * Inputs: atoms [B,N] u8 labels, bonds [B,cap,4] u8 rows (hi, lo, label, 0) (4-byte aligned), n_bonds [B], as dg_decode_graph
 * wrote them; of dg_mol_descriptors' outputs desc [B,DG_DESC_FIELDS] i32 (only the status, entry 0, is read), atom_key [B,N]
 * u32 and bond_class [B,cap] u8; and bond_table [n_bond_labels] u32: order | aromatic << 8, the table of dg_mol_validity.
 *
 * The scope is derived, not passed, exactly as dg_mol_substructure derives it.  status[b] = desc[b,0].  For a molecule of
 * status 0:
 *   an atom a is in the scope iff atom_key[b,a] != DG_DESC_NO_KEY;
 *   a row k < min(n_bonds, cap) of the bond list is a BOND iff bond_class[b,k] & DG_DESC_BOND, and a RING BOND iff it is a BOND
 *   and bond_class[b,k] & DG_DESC_RING_BOND.
 * Arrays outside the definition (a record of another batch, a table of other decoders): the result then has no meaning, but the
 * kernel stays inside its arrays.  A row with an end >= N, with hi == lo, with an end outside the scope, or whose label is
 * >= n_bond_labels or has an UNKNOWN table word (order 0 or > 3, bits above 8, aromatic with order != 1) is skipped: it is no
 * BOND.  The decode lists no pair twice; a list that does is outside the definition.
 *
 * Definition, for a molecule of status 0 (any other status gives the EMPTY RESULT below):
 *   CORE          the largest set of scope atoms in which every atom has at least two BONDS to other atoms of the set: what is
 *                 left when atoms with at most one BOND to a remaining atom are removed until none is.  Ring atoms and the
 *                 linkers between rings; an acyclic molecule has an empty core.
 *   EXO ATOM      a scope atom outside the core with a BOND of table order 2, not aromatic, to a core atom.  Only that atom is
 *                 kept, not what hangs on it: a ring C=O keeps its O, a ring =C(C)C keeps one C.  An exo atom has exactly one
 *                 BOND to the core and none to another exo atom (either would have kept it in the core).
 *   SCAFFOLD      the core and the exo atoms, with every BOND whose two ends are both scaffold atoms.
 *   role[a]       DG_SCAF_ROLE_NONE outside the scope; else _RING if a has a RING BOND; else _LINKER if a is in the core; else
 *                 _EXO if a is an exo atom; else _SIDE.
 *   RING SYSTEM   a connected component of the graph of the RING BONDS; system[a] = the smallest atom index of a's system,
 *                 DG_SCAF_NO_SYSTEM if a has no RING BOND.
 *   ring size of a RING BOND (i, j): 1 + the number of BONDS of the shortest path from i to j that does not use the bond
 *                 itself, saturated at DG_SCAF_MAX_RING (a 256-cycle reads 255; so does a row that claims to be a RING BOND
 *                 and has no such path, which is outside the definition).
 *
 * Outputs, every element stored by every call but the rows of bond_ring_size and s_bonds named below:
 *   mol [B,16] i32: status; and for status 0 -- all of them 0 otherwise --
 *        1 n_heavy                the atoms of the scope;
 *        2 n_scaffold_atoms       3 n_scaffold_bonds       4 n_exo       5 n_linker_atoms
 *        6 n_ring_atoms           the atoms with a RING BOND;            7 n_ring_bonds
 *        8 n_rings                n_ring_bonds - n_ring_atoms + n_ring_systems (the cyclomatic number: dg_mol_descriptors' n_rings);
 *        9 n_ring_systems        10 largest_system_atoms   the atoms of the ring system with the most atoms;
 *       11 min_ring              12 max_ring               the smallest and largest ring size of a RING BOND, 0 without one;
 *       13..15                    0.
 *   ring_hist [B,8] i32: the RING BONDS by ring size, in the bins 3, 4, 5, 6, 7, 8, 9..12, >= 13.
 *   atom_role [B,N] u8, atom_system [B,N] u8: as above.
 *   bond_ring_size [B,cap] u8: for the first min(n_bonds, cap) rows the ring size of a RING BOND, 0 for every other row.  The
 *       entries past min(n_bonds, cap) are not touched.
 *   The derived batch -- exactly what dg_decode_graph would have written for the scaffold graph on the same N and cap:
 *     s_atoms [B,N] u8             the label of a scaffold atom, 0 at every other position;
 *     s_bonds [B,cap,4] u8         the rows of the scaffold's BONDS (hi, lo, label, 0) in their order in `bonds`, compacted to
 *                                  the front; the rows past s_n_bonds are not touched;
 *     s_n_bonds [B] i32            n_scaffold_bonds (never more than cap);
 *     s_component [B,N] u8         the smallest atom index of the atom's connected component in the scaffold graph (an atom
 *                                  outside the scaffold is a component of its own);
 *     s_n_components, s_largest, s_largest_size [B] i32   the component count, the component with the most atoms (ties: the
 *                                  smaller index) and its atom count.
 *   The EMPTY RESULT (status != 0, and equally an acyclic molecule's derived batch): mol = (status, 0, ...), ring_hist 0,
 *   atom_role 0, atom_system DG_SCAF_NO_SYSTEM, bond_ring_size 0 over the first min(n_bonds, cap) rows, s_atoms 0, s_n_bonds 0,
 *   s_component[a] = a, s_n_components = N, s_largest = 0, s_largest_size = 1.
 * All outputs are functions of the input alone: pinned values.
 *
 * B < 0, N outside 1..256, cap < 0 or n_bond_labels outside 1..256: DG_E_SHAPE; a null pointer (bonds, bond_class,
 * bond_ring_size and s_bonds may be NULL when cap == 0) or a misaligned one (bonds, n_bonds, desc, atom_key, bond_table, mol,
 * ring_hist, s_bonds, s_n_bonds, s_n_components, s_largest, s_largest_size: 4 bytes): DG_E_ARG.  The shape is checked first.
 * B == 0 returns 0 without a launch. */
int dg_mol_scaffold(const unsigned char* atoms, const unsigned char* bonds, const int* n_bonds, const int* desc,
                    const unsigned* atom_key, const unsigned char* bond_class, const unsigned* bond_table, int n_bond_labels,
                    int B, int N, int cap, int* mol, int* ring_hist, unsigned char* atom_role, unsigned char* atom_system,
                    unsigned char* bond_ring_size, unsigned char* s_atoms, unsigned char* s_bonds, int* s_n_bonds,
                    unsigned char* s_component, int* s_n_components, int* s_largest, int* s_largest_size, dg_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* DRUGGEN_HIP_SCAF_H */
