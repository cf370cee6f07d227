"""Substructure patterns on decoded molecules, matched on the GPU (``dg_mol_substructure``, ``include/druggen_hip_sub.h``, DESIGN
3.32): how many atoms each pattern of a table matches at -- functional groups, alerts -- and an ordered first-match atom typing
whose additive values give a Wildman-Crippen style logP, and with it the last of Lipinski's rules (``lipinski_rules5``).  The
consumer of ``descriptors.describe_molecules``' ``atom_key`` and ``bond_class``: no device->host copy of the molecules, no RDKit.

The header states the matcher in full.  It is the project's own and NOT RDKit's SMARTS engine: patterns are written in the small
grammar of ``parse_pattern``, the search is bounded (``MAX_STEPS`` steps per pattern and anchor, then the pair counts as no match
and in ``n_over``), and a pattern's count is the number of ANCHOR atoms it matches at, not the number of matches.  The built-in
typing table ``LOGP`` is a REDUCED table in the style of Wildman and Crippen (1999), WRITTEN DOWN FROM MEMORY as the ``TPSA``
table of ``descriptors`` is: its rows and values are not the published ones, and how far ``logp`` sits from
``Crippen.MolLogP`` has not been measured (RDKit is not available where this was built).  Bring your own rows with ``typing=``.
There is no PAINS catalogue here: it cannot be reproduced from memory; a user brings its patterns in the text form.  GPU only, no
CPU fallback."""
from __future__ import annotations

import numpy as np
import torch

from . import _lib
from ._packed import PackedRecord
from .canon import _scope_code
from .decode import decode_molecule_graphs, device_batch
from .descriptors import DescriptorTables, MoleculeDescriptors
from .descriptors import _launch as _describe
from .smiles import _Z
from .smiles_out import table_rows as _symbol_rows
from .validity import _ORDER, VALID, MoleculeValidity, ValenceTables
from .validity import _launch as _check

__all__ = ["Pattern", "parse_pattern", "pack_pattern", "unpack_pattern", "SubstructureTables", "MoleculeMatches", "match_molecules",
           "match_store", "lipinski_rules5", "LOGP", "GROUPS", "MOL_FIELDS", "MAX_ATOMS", "MAX_CLOSURES", "MAX_PATTERNS",
           "MAX_STEPS", "PATTERN_WORDS", "TYPING"]

MOL_FIELDS = ("status", "n_heavy", "n_typed", "n_untyped", "sum0", "sum1", "n_patterns_hit", "n_over")      # the row of `mol`
MAX_ATOMS, MAX_CLOSURES, MAX_PATTERNS, MAX_STEPS, PATTERN_WORDS, TYPING = 16, 8, 1024, 4096, 80, 1
_WIDTH = dict(h=9, deg=9, n2=5, n3=3, arom=2, ring=2, r3=2)      # bits of each allowed-value mask
_KINDS = {"-": 0, "=": 1, "#": 2, ":": 3}
_DEFAULT_BOND = 0x99      # an omitted bond: `-,:`, in a ring or not

# The built-in typing table: (name, pattern, value, value_h) in 1e-4 log units, first match wins.  A REDUCED table in the style of
# Wildman and Crippen, J. Chem. Inf. Comput. Sci. 39 (1999) 868, written down FROM MEMORY: fewer rows than the published 68, and
# the values are recollections, not a transcription.  value_h is the contribution of every hydrogen on the atom (the published
# scheme types hydrogens by their carrier: on carbon, on nitrogen, of an alcohol, of an acid).  Every element ends in a catch-all
# row, so that a valid molecule of C, N, O, F, P, S, Cl, Br and I has no untyped atom.
LOGP = (
    ("C.ar.fused", "[C;a;D3](:[*])(:[*]):[*]", 2955, 1230),       # aromatic carbon at a ring fusion
    ("C.ar.hetero", "[C;a;D3]-[!C]", 1129, 1230),                 # aromatic carbon with a hetero substituent
    ("C.ar.subst", "[C;a;D3]", 1360, 1230),                       # aromatic carbon with a carbon substituent
    ("C.ar", "[C;a]", 1581, 1230),                                # aromatic CH
    ("C.triple", "[C;T1,2]", 17, 1230),                           # carbon of a triple bond
    ("C.dbl.hetero", "[C]=[!C]", -2783, 1230),                    # C=X
    ("C.dbl", "[C;Y1,2]", 1551, 1230),                            # C=C
    ("C.sp3.hetero", "[C]-[!C]", -2035, 1230),                    # saturated carbon on a hetero atom
    ("C.sp3.branched", "[C;H0,1]", 0, 1230),                      # CHR3, CR4
    ("C", "[C]", 1441, 1230),                                     # CH4, CH3R, CH2R2; every other carbon
    ("N.ar", "[N;a]", -3239, 2142),                               # aromatic nitrogen
    ("N.triple", "[N;T1]", -5660, 2142),                          # nitrile nitrogen
    ("N.dbl", "[N;Y1,2]", -1390, 2142),                           # imine nitrogen
    ("N.aryl", "[N]-[C;a]", -5188, 2142),                         # amine on an aromatic carbon
    ("N.primary", "[N;H2,3]", -10190, 2142),
    ("N.secondary", "[N;H1]", -7096, 2142),
    ("N", "[N]", -10270, 2142),                                   # tertiary amine; every other nitrogen
    ("O.ar", "[O;a]", 1552, 0),                                   # aromatic oxygen
    ("O.carbonyl", "[O;Y1]", -3339, 0),                           # =O
    ("O.acid", "[O;H1]-[C]=[O]", -2893, 2980),                    # the OH of an acid
    ("O.hydroxyl", "[O;H1,2]", -2893, -2677),                     # alcohol, phenol, water
    ("O", "[O]", -684, 0),                                        # ether; every other oxygen
    ("F", "[F]", 4202, 0),
    ("P", "[P]", 8612, 1230),
    ("S.ar", "[S;a]", 6237, 0),
    ("S", "[S]", 6482, 1230),
    ("Cl", "[Cl]", 6895, 0),
    ("Br", "[Br]", 8456, 0),
    ("I", "[I]", 8857, 0),
)

# The built-in counted patterns: (name, pattern), each anchored at its distinctive atom, so that the anchor count is the group count
GROUPS = (
    ("amide", "[C;Y1](=[O])-[N]"),                                 # the carbonyl carbon
    ("ester", "[C;Y1](=[O])-[O;H0]-[C]"),
    ("carboxylic_acid", "[C;Y1](=[O])-[O;H1]"),
    ("nitrile", "[C;T1]#[N]"),
    ("primary_amine", "[N;H2;A;Y0]-[C;Y0;T0]"),                    # amines: a saturated nitrogen on carbons that carry no C=X
    ("secondary_amine", "[N;H1;A;D2;Y0](-[C;Y0;T0])-[C;Y0;T0]"),
    ("tertiary_amine", "[N;H0;A;D3;Y0](-[C;Y0;T0])(-[C;Y0;T0])-[C;Y0;T0]"),
    ("aryl_halide", "[F,Cl,Br,I]-[C;a]"),
    ("alcohol", "[O;H1]-[C;A;Y0]"),
    ("ether", "[O;H0;D2;A](-[C;Y0])-[C;Y0]"),                      # no ester oxygen
    ("ketone", "[C;Y1](=[O])(-[C])-[C]"),
    ("enone", "[C;Y1](=[O])-[C]=[C]"),                             # an alpha,beta-unsaturated carbonyl
)


class Pattern:
    """A parsed pattern: ``atoms`` -- per atom a dict of ``elements`` (a frozenset of atomic numbers, or None for ``*``),
    ``negate``, the masks ``h``, ``deg``, ``n2``, ``n3``, ``arom``, ``ring``, ``r3``, and for atoms after the first ``parent``
    and ``bond`` (the 8-bit mask of admitted kinds) -- in writing order, which is the depth-first preorder; ``closures`` --
    ``(k, j, mask)`` with ``j < k``, sorted by ``k``."""

    def __init__(self, atoms, closures, text=""):
        self.atoms, self.closures, self.text = atoms, closures, text

    def __repr__(self):
        return f"Pattern({self.text!r}: {len(self.atoms)} atoms, {len(self.closures)} closures)"


def _number_list(text, what, top):
    mask = 0
    for item in text.split(","):
        if not item.isdigit():
            raise ValueError(f"unsupported: {what!r} takes a comma list of values, got {what + text!r}")
        if int(item) > top:
            raise ValueError(f"unsupported: {what}{item} -- values of {what!r} go up to {top}")
        mask |= 1 << int(item)
    return mask


def _parse_atom(body, text):
    if body == "":
        raise ValueError(f"unsupported: an empty bracket atom in {text!r}")
    for sign, name in (("$", "a recursive environment $()"), ("+", "a charge"), ("@", "chirality"), ("&", "the & operator"),
                       ("^", "hybridisation")):
        if sign in body:
            raise ValueError(f"unsupported: {name} in [{body}] of {text!r}")
    if body[0].isdigit():
        raise ValueError(f"unsupported: an isotope in [{body}] of {text!r}")
    if ":" in body:
        raise ValueError(f"unsupported: an atom map in [{body}] of {text!r}")
    atom = dict(elements=None, negate=False, **{k: (1 << w) - 1 for k, w in _WIDTH.items()})
    seen_elements = False
    for item in body.split(";"):
        if item == "":
            raise ValueError(f"unsupported: an empty constraint in [{body}] of {text!r}")
        if item in ("a", "A"):
            atom["arom"] &= 2 if item == "a" else 1
        elif item in ("R", "!R"):
            atom["ring"] &= 2 if item == "R" else 1
        elif item in ("r3", "!r3"):
            atom["r3"] &= 2 if item == "r3" else 1
        elif item[0] in "HDYT" and len(item) > 1 and item[1].isdigit():
            field, top = {"H": ("h", 8), "D": ("deg", 8), "Y": ("n2", 4), "T": ("n3", 2)}[item[0]]
            atom[field] &= _number_list(item[1:], item[0], top)
        elif item == "*":
            seen_elements = True
        else:
            if "-" in item:
                raise ValueError(f"unsupported: a charge in [{body}] of {text!r}")
            negate = item.startswith("!")
            numbers = set()
            for sym in item[negate:].split(","):
                if sym.startswith("#") and sym[1:].isdigit() and 1 <= int(sym[1:]) <= 118:
                    numbers.add(int(sym[1:]))
                elif sym in _Z and sym != "H":      # (`H` alone is no hydrogen count: write H1)
                    numbers.add(_Z[sym])
                else:
                    raise ValueError(f"unsupported: the constraint {item!r} in [{body}] of {text!r} (an element list by symbol or "
                                     "#Z, H / D / Y / T with values, a / A, R / !R, r3 / !r3 or *)")
            if seen_elements or atom["elements"] is not None:
                raise ValueError(f"unsupported: two element constraints in [{body}] of {text!r}")
            atom["elements"], atom["negate"] = frozenset(numbers), negate
    return atom


def _parse_bond(text, at, whole):
    """The bond mask written at ``text[at:]`` and the index behind it; None if there is no bond symbol."""
    start, kinds = at, 0
    while at < len(text) and text[at] in "-=#:~":
        kinds |= 15 if text[at] == "~" else 1 << _KINDS[text[at]]
        at += 1
        if at < len(text) and text[at] == ",":
            at += 1
            if at >= len(text) or text[at] not in "-=#:~":
                raise ValueError(f"unsupported: a bond list must go on with a bond symbol, at {at} of {whole!r}")
            continue
        break
    if at == start:
        if text.startswith("@", at) or text.startswith("!@", at):
            raise ValueError(f"unsupported: a ring suffix without a bond symbol (write ~@), at {at} of {whole!r}")
        return None, at
    mask = kinds | kinds << 4
    if text.startswith("!@", at):
        mask, at = mask & 0x0F, at + 2
    elif text.startswith("@", at):
        mask, at = mask & 0xF0, at + 1
    return mask, at


def parse_pattern(text):
    """Parse a pattern of this module's own grammar -- a small, exactly stated SMARTS-like SUBSET, not SMARTS -- into a
    ``Pattern``.

    Every atom is a bracket atom, ``[`` constraints joined by ``;`` ``]``, all of which must hold:
      * an element list ``C,N,#16`` by symbol or ``#Z``, with an optional leading ``!`` that negates the whole list, or ``*``
        for any element (at most one of these per atom; none means ``*``);
      * ``H``, ``D`` (neighbours in the graph), ``Y`` (double bonds) and ``T`` (triple bonds), each followed by a comma list of
        allowed values: ``H0``, ``D2,3``; H and D 0..8, Y 0..4, T 0..2;
      * ``a`` / ``A`` (has / has no aromatic bond), ``R`` / ``!R`` (has / has no ring bond), ``r3`` / ``!r3`` (in / outside a
        three-ring).
    Bonds: ``-`` ``=`` ``#`` ``:`` ``~`` (any) and comma lists of them, with an optional suffix ``@`` (a ring bond) or ``!@`` (not
    one); an omitted bond means ``-,:``.  Branches in ``( )``; ring-closure digits 1-9, where the bond of the closure is written
    at its SECOND digit and belongs to that, later, atom.  The writing order is the depth-first preorder the matcher follows.

    Anything else raises ``ValueError`` naming the unsupported feature: bare atoms outside brackets, charges, recursive ``$()``,
    isotopes, chirality, atom maps, ``&``, ``.``, ``%nn`` closures, more than 16 atoms, more than 8 closures."""
    if not isinstance(text, str) or not text:
        raise ValueError(f"unsupported: a pattern is a non-empty string, got {text!r}")
    atoms, closures, open_rings, stack = [], [], {}, []
    last, at, pending = None, 0, None
    while at < len(text):
        ch = text[at]
        if ch == "[":
            end = text.find("]", at)
            if end < 0:
                raise ValueError(f"unsupported: an unclosed bracket in {text!r}")
            atom = _parse_atom(text[at + 1:end], text)
            if last is None and atoms:
                raise ValueError(f"unsupported: a second component in {text!r}")
            if last is not None:
                atom["parent"], atom["bond"] = last, _DEFAULT_BOND if pending is None else pending
            elif pending is not None:
                raise ValueError(f"unsupported: a bond before the first atom of {text!r}")
            atoms.append(atom)
            if len(atoms) > MAX_ATOMS:
                raise ValueError(f"unsupported: more than {MAX_ATOMS} atoms in {text!r}")
            last, pending, at = len(atoms) - 1, None, end + 1
        elif ch == "(":
            if last is None or pending is not None:
                raise ValueError(f"unsupported: a branch without an atom before it, at {at} of {text!r}")
            stack.append(last)
            at += 1
        elif ch == ")":
            if not stack or pending is not None:
                raise ValueError(f"unsupported: an unmatched ')' at {at} of {text!r}")
            last = stack.pop()
            at += 1
        elif ch.isdigit():
            if last is None or ch == "0":
                raise ValueError(f"unsupported: the ring-closure digit at {at} of {text!r} (digits 1-9 after an atom)")
            if ch in open_rings:
                first = open_rings.pop(ch)
                if first == last:
                    raise ValueError(f"unsupported: a ring closure of an atom with itself in {text!r}")
                closures.append((last, first, _DEFAULT_BOND if pending is None else pending))
                if len(closures) > MAX_CLOSURES:
                    raise ValueError(f"unsupported: more than {MAX_CLOSURES} ring closures in {text!r}")
            else:
                if pending is not None:
                    raise ValueError(f"unsupported: a bond at the opening digit of a ring closure (write it at the closing "
                                     f"digit), at {at} of {text!r}")
                open_rings[ch] = last
            pending, at = None, at + 1
        elif ch == "%":
            raise ValueError(f"unsupported: %nn ring closures in {text!r}")
        elif ch == ".":
            raise ValueError(f"unsupported: a disconnected pattern ('.') in {text!r}")
        elif ch in "/\\":
            raise ValueError(f"unsupported: a directional bond in {text!r}")
        else:
            if pending is not None:
                raise ValueError(f"unsupported: two bonds in a row at {at} of {text!r}")
            pending, nxt = _parse_bond(text, at, text)
            if pending is None:
                raise ValueError(f"unsupported: {ch!r} at {at} of {text!r} (every atom is a bracket atom)")
            at = nxt
    if not atoms:
        raise ValueError(f"unsupported: a pattern without an atom, {text!r}")
    if stack or open_rings or pending is not None:
        raise ValueError(f"unsupported: an open branch, ring closure or bond at the end of {text!r}")
    return Pattern(atoms, sorted(closures, key=lambda c: c[0]), text)


def pack_pattern(pattern, element_bits, flags=0, values=(0, 0, 0, 0)):
    """The ``PATTERN_WORDS`` uint32 record of a ``Pattern`` (the layout is in the header).  ``element_bits``: atomic number ->
    set bit of ``atom_sets``; an element without a bit contributes nothing, ``*`` and a negated list are taken within the bits
    there are.  ``values``: ``(value[0], value_h[0], value[1], value_h[1])``, int32."""
    every = 0
    for bit in element_bits.values():
        every |= 1 << bit
    rec = np.zeros(PATTERN_WORDS, dtype=np.uint32)
    rec[0] = len(pattern.atoms) | len(pattern.closures) << 8 | int(flags) << 16
    for k, v in enumerate(values):
        if not -(1 << 31) <= int(v) < 1 << 31:
            raise ValueError(f"a pattern value must fit an int32, got {v}")
        rec[1 + k] = int(v) & 0xFFFFFFFF
    for k, a in enumerate(pattern.atoms):
        named = 0
        for z in a["elements"] or ():
            if z in element_bits:
                named |= 1 << element_bits[z]
        sets = every if a["elements"] is None else every & ~named if a["negate"] else named
        rec[8 + 4 * k:12 + 4 * k] = (sets, a["h"] | a["deg"] << 16, a["n2"] | a["n3"] << 8 | a["arom"] << 12 | a["ring"] << 14
                                     | a["r3"] << 16, (a["parent"] | a["bond"] << 8) if k else 0)
    for i, (k, j, mask) in enumerate(pattern.closures):
        rec[72 + i] = k | j << 8 | mask << 16
    return rec


def unpack_pattern(rec):
    """The fields of a record: ``dict(n, flags, values, atoms=[dict(sets, h, deg, n2, n3, arom, ring, r3, parent, bond)],
    closures=[(k, j, mask)])``."""
    rec = [int(x) for x in rec]
    n, c = rec[0] & 255, (rec[0] >> 8) & 255
    atoms = []
    for k in range(n):
        w = rec[8 + 4 * k:12 + 4 * k]
        atoms.append(dict(sets=w[0], h=w[1] & 0x1FF, deg=(w[1] >> 16) & 0x1FF, n2=w[2] & 31, n3=(w[2] >> 8) & 7, arom=(w[2] >> 12) & 3,
                          ring=(w[2] >> 14) & 3, r3=(w[2] >> 16) & 3, parent=w[3] & 255, bond=(w[3] >> 8) & 255))
    return dict(n=n, flags=rec[0] >> 16, values=tuple(v - (1 << 32) if v >> 31 else v for v in rec[1:5]), atoms=atoms,
                closures=[(w & 255, (w >> 8) & 255, (w >> 16) & 255) for w in rec[72:72 + c]])


class SubstructureTables:
    """The tables of ``dg_mol_substructure`` on a device; the kernel itself knows no chemistry.  ``names``: the patterns in table
    order, the ``n_typing`` typing rows first; ``pattern_rows`` ``[n_patterns, 80]`` uint32; ``atom_set_rows`` ``[n_atom_labels]``
    uint32 (one bit per distinct element of the decoder, ``element_bits``); ``bond_rows`` ``[n_bond_labels]`` (``order |
    aromatic << 8``, the validity check's)."""

    def __init__(self, names, pattern_rows, atom_sets, bond_rows, device, n_typing=0, element_bits=None):
        pattern_rows = np.ascontiguousarray(pattern_rows, dtype=np.uint32).reshape(-1, PATTERN_WORDS)
        atom_sets, bond_rows = (np.ascontiguousarray(t, dtype=np.uint32) for t in (atom_sets, bond_rows))
        names = tuple(names)
        if len(pattern_rows) > MAX_PATTERNS:
            raise ValueError(f"the pattern table has {len(pattern_rows)} rows, at most {MAX_PATTERNS} fit")
        if len(names) != len(pattern_rows) or len(set(names)) != len(names):
            raise ValueError("one name per pattern, and no name twice")
        if atom_sets.ndim != 1 or not 1 <= len(atom_sets) <= 255:
            raise ValueError("atom_sets is one word per atom label, 1..255 labels")
        if bond_rows.ndim != 1 or not 1 <= len(bond_rows) <= 256:
            raise ValueError("bond_rows is one word per bond label, 1..256 labels")
        self.names, self.index = names, {name: k for k, name in enumerate(names)}
        self.pattern_rows, self.atom_set_rows, self.bond_rows = pattern_rows, atom_sets, bond_rows
        self.n_patterns, self.n_typing, self.n_atom_labels, self.n_bond_labels = len(names), int(n_typing), len(atom_sets), len(bond_rows)
        self.element_bits = dict(element_bits or {})

        def up(a):
            return torch.from_numpy(a.view(np.int32)).to(device).contiguous()      # (the bit patterns)
        self.patterns, self.atom_sets, self.bonds = up(pattern_rows), up(atom_sets), up(bond_rows)
        self.device = self.atom_sets.device      # with its index, as a batch's buffer reports it

    @classmethod
    def from_decoders(cls, atom_decoder, bond_decoder, device, typing=None, patterns=None):
        """Build and upload the tables.  ``typing``: None for the built-in ``LOGP``, else rows ``(name, text, value, value_h[,
        value1, value_h1])`` -- they come first, in the given order, which is the order of the first-match typing; ``patterns``:
        None for the built-in ``GROUPS``, else counted rows ``(name, text)``, which follow.  One set bit per distinct element of
        the atom decoder (the pad, atomic number 0, has none); ``ValueError`` on more than 32 distinct elements, more than 1024
        patterns, a name twice, and whatever ``parse_pattern`` refuses.  The decoders are those of
        ``SmilesTables.from_decoders``, checked like them."""
        _symbol_rows(atom_decoder, bond_decoder)
        z = [int(atom_decoder[l]) for l in range(len(atom_decoder))]
        elements = sorted({a for a in z if a != 0})
        if len(elements) > 32:
            raise ValueError(f"the atom decoder names {len(elements)} distinct elements, at most 32 fit the set word")
        bits = {a: k for k, a in enumerate(elements)}
        typing = LOGP if typing is None else tuple(typing)
        counted = GROUPS if patterns is None else tuple(patterns)
        if len(typing) + len(counted) > MAX_PATTERNS:
            raise ValueError(f"{len(typing) + len(counted)} patterns, at most {MAX_PATTERNS} fit")
        names, rows = [], []
        for row in typing:
            if len(row) not in (4, 6):
                raise ValueError(f"a typing= row is (name, text, value, value_h[, value1, value_h1]), got {row!r}")
            names.append(row[0])
            rows.append(pack_pattern(parse_pattern(row[1]), bits, TYPING, tuple(row[2:]) + (0, 0) * (len(row) == 4)))
        for row in counted:
            if len(row) != 2:
                raise ValueError(f"a patterns= row is (name, text), got {row!r}")
            names.append(row[0])
            rows.append(pack_pattern(parse_pattern(row[1]), bits))
        if len(set(names)) != len(names):
            raise ValueError(f"a pattern name occurs twice: {sorted(n for n in set(names) if names.count(n) > 1)}")
        table = np.stack(rows) if rows else np.zeros((0, PATTERN_WORDS), dtype=np.uint32)
        return cls(names, table, [1 << bits[a] if a else 0 for a in z],
                   [_ORDER.get(int(bond_decoder[l]), 0) for l in range(len(bond_decoder))], device, len(typing), bits)


class MoleculeMatches(PackedRecord):
    """The matches of one batch: typed views of one packed byte buffer.

    ====================  ====================  ======================================================================
    ``mol``               [B,8] int32           one row per molecule; its columns are the attributes below
    ``status``            [B] int32             the validity status; every other column is 0 unless it is 0
    ``n_heavy``           [B] int32             atoms of the scope
    ``n_typed``, ``n_untyped`` [B] int32        scope atoms with / without a typing row
    ``sum0``, ``sum1``    [B] int32             the sums of the typing values (and of ``h`` x the hydrogen values)
    ``n_patterns_hit``    [B] int32             patterns that match somewhere
    ``n_over``            [B] int32             (pattern, anchor) searches given up at ``MAX_STEPS``: they count as no match
    ``hits``              [B,n_patterns] int32  per pattern the number of atoms it matches at (anchors, not matches)
    ``atom_type``         [B,N] int32           the first typing row that matches at the atom; -1: none, outside the scope,
                                                or status != 0
    ====================  ====================  ======================================================================

    ``names`` are the table's pattern names (``count(name)`` is a column of ``hits``).  ``cpu()`` moves the packed buffer with
    ONE device->host copy."""

    names = ()

    def __init__(self, buffer, B, N, n_patterns, names=()):
        self.B, self.N, self.n_patterns = B, N, n_patterns
        super().__init__(buffer, B, N, n_patterns)
        self.names = tuple(names)

    @staticmethod
    def _fields(B, N, n_patterns):
        return ("mol", 4, (B, len(MOL_FIELDS))), ("hits", 4, (B, n_patterns)), ("atom_type", 4, (B, N))

    @staticmethod
    def empty(B, N, n_patterns, device, names=()):
        """A device record over an uninitialised buffer (``match_molecules(..., out=)`` fills it)."""
        rec = MoleculeMatches._empty(device, B, N, n_patterns)
        rec.names = tuple(names)
        return rec

    def __len__(self):
        return self.B

    def count(self, name):
        """``hits[:, p]`` of the pattern called ``name``: int32 [B]."""
        try:
            return self.hits[:, self.names.index(name)]
        except ValueError:
            raise KeyError(f"no pattern is called {name!r}") from None

    @property
    def logp(self):
        """``sum0 / 1e4``, float64 [B]: the logP of the typing table (see the module's text for what it is not)."""
        return self.sum0.astype(np.float64) / 1e4 if self.is_host else self.sum0.to(torch.float64) / 1e4


for _k, _name in enumerate(MOL_FIELDS):
    setattr(MoleculeMatches, _name, property(lambda self, _k=_k: self.mol[:, _k]))


def _launch(batch, descriptors, tables, out, at=0, seen=0):
    """``dg_mol_substructure`` of ``batch`` into the rows ``at ..`` of ``out``, its keys and classes read from the rows
    ``seen ..`` of ``descriptors``."""
    if batch.B == 0:
        return
    cap, n = batch.cap, tables.n_patterns
    _lib.launch("dg_mol_substructure", batch.buffer,
                batch.atoms.data_ptr(), batch.bonds.data_ptr() if cap > 0 else None, batch.n_bonds.data_ptr(),
                descriptors.desc[seen:].data_ptr(), descriptors.atom_key[seen:].data_ptr(),
                descriptors.bond_class[seen:].data_ptr() if cap > 0 else None, tables.bonds.data_ptr(), tables.n_bond_labels,
                tables.atom_sets.data_ptr(), tables.n_atom_labels, tables.patterns.data_ptr() if n else None, n, batch.B, batch.N,
                cap, out.mol[at:].data_ptr(), out.hits[at:].data_ptr() if n else None, out.atom_type[at:].data_ptr())


def _check_tables(tables, who, dev):
    if not isinstance(tables, SubstructureTables):
        raise TypeError(f"{who} takes SubstructureTables (SubstructureTables.from_decoders)")
    if tables.device != dev:
        raise ValueError(f"the tables live on {tables.device}, the molecules on {dev}")


def match_molecules(batch, descriptors, tables, out=None):
    """``MoleculeMatches`` of a device ``MoleculeBatch``, on its device and the current stream.

    ``descriptors``: the ``MoleculeDescriptors`` that ``describe_molecules`` made of THIS batch (its status, ``atom_key`` and
    ``bond_class`` are read on the device, and they carry the scope; another batch's record gives numbers without a meaning).
    ``out``: a ``MoleculeMatches.empty(B, N, n_patterns, device)`` to write into.  One launch; every element is written by
    every call, nothing is allocated with ``out=`` and nothing synchronises: capturable."""
    device_batch(batch, "match_molecules", "substructure")
    dev = batch.buffer.device
    _check_tables(tables, "match_molecules", dev)
    B, N, cap = batch.B, batch.N, batch.cap
    if (not isinstance(descriptors, MoleculeDescriptors) or descriptors.is_host or (descriptors.B, descriptors.N, descriptors.cap) != (B, N, cap)
            or descriptors.buffer.device != dev):
        raise ValueError("descriptors= must be the device MoleculeDescriptors of this batch (descriptors.describe_molecules)")
    if out is None:
        out = MoleculeMatches.empty(B, N, tables.n_patterns, dev, tables.names)
    elif (not isinstance(out, MoleculeMatches) or out.is_host or (out.B, out.N, out.n_patterns) != (B, N, tables.n_patterns)
            or out.buffer.device != dev):
        raise ValueError("out= must be a device MoleculeMatches of this batch's B and N and the tables' pattern count "
                         "(MoleculeMatches.empty)")
    out.names = tables.names
    _launch(batch, descriptors, tables, out)
    return out


def match_store(store, valence_tables, descriptor_tables, tables, chunk=1024, scope="largest", bond_cap=None):
    """``(MoleculeValidity, MoleculeDescriptors, MoleculeMatches)`` of every molecule of a ``resident.ResidentMolecules`` store,
    ``chunk`` molecules at a time by the route of ``descriptors.descriptor_store``: ``store.batch`` ->
    ``decode_molecule_graphs`` -> ``dg_mol_validity`` -> ``dg_mol_descriptors`` -> ``dg_mol_substructure``, each written at the
    row offsets of one record.  Nothing but the unwritten rows past a molecule's bond count depends on ``chunk``."""
    code = _scope_code(scope)
    chunk = int(chunk)
    if chunk < 1:
        raise ValueError(f"chunk must be >= 1, got {chunk}")
    if not isinstance(valence_tables, ValenceTables) or not isinstance(descriptor_tables, DescriptorTables):
        raise TypeError("match_store takes ValenceTables, DescriptorTables and SubstructureTables (their from_decoders)")
    _check_tables(tables, "match_store", store.device)
    for other in (valence_tables, descriptor_tables):
        if other.device != tables.device:
            raise ValueError(f"the {type(other).__name__} live on {other.device}, the molecules on {tables.device}")
    n, N = len(store), store.vertexes
    cap = N * (N - 1) // 2 if bond_cap is None else int(bond_cap)
    checked = MoleculeValidity.empty(n, N, cap, store.device)
    described = MoleculeDescriptors.empty(n, N, cap, store.device)
    out = MoleculeMatches.empty(n, N, tables.n_patterns, store.device, tables.names)
    for at in range(0, n, chunk):
        index = torch.arange(at, min(n, at + chunk), device=store.device)
        _, a, x = store.batch(index)
        if store.atom_dim != store.m_dim:
            x = x[..., :store.atom_dim].contiguous()
        batch = decode_molecule_graphs(x, a, bond_cap=cap)
        _check(batch, valence_tables, code, checked, at)
        _describe(batch, checked, descriptor_tables, code, described, at, at)
        _launch(batch, described, tables, out, at, at)
    return checked, described, out


def lipinski_rules5(validity, descriptors, matches):
    """How many of five rules each molecule obeys, int32 [B] in 0..5: the four of ``descriptors.lipinski_rules`` (mass < 500 Da,
    donors <= 5, acceptors <= 10, ``n_rot <= 10``) and ``-2 <= logP <= 5`` with ``matches.logp`` -- the reference's
    ``obey_lipinski``.  The logP rule counts only where the typing is complete: ``n_untyped == 0`` and ``n_over == 0``.  0 for a
    molecule whose status is not 0.  The reference's own line, ``(logp := MolLogP(mol) >= -2) & (logp <= 5)``, binds the walrus
    to the comparison, so ``logp`` there is a bool and the line only ever tests the lower bound; both bounds are tested here.
    ``logp`` is the built-in ``LOGP`` table's (or the caller's ``typing=``), a reduced table written from memory and not
    ``Crippen.MolLogP``; the other four rules are as ``descriptors.lipinski_rules`` documents them."""
    v, d, m = validity, descriptors, matches
    if (not isinstance(v, MoleculeValidity) or not isinstance(d, MoleculeDescriptors) or not isinstance(m, MoleculeMatches)
            or not v.is_host == d.is_host == m.is_host or not v.B == d.B == m.B):
        raise ValueError("lipinski_rules5 takes a MoleculeValidity and the MoleculeDescriptors and MoleculeMatches made from it, "
                         "all on the device or all on the host")
    logp_ok = (m.sum0 >= -20000) & (m.sum0 <= 50000) & (m.n_untyped == 0) & (m.n_over == 0)
    rules = (v.mass < 5000000, v.n_donors <= 5, v.n_acceptors <= 10, d.n_rot <= 10, logp_ok)
    valid = d.status == VALID
    if d.is_host:
        return np.where(valid, sum(r.astype(np.int32) for r in rules), 0).astype(np.int32)
    total = sum(r.to(torch.int32) for r in rules)
    return torch.where(valid, total, torch.zeros_like(total))
