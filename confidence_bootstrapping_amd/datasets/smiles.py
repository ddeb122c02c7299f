"""Ligands written as SMILES, without rdkit: `mol_from_smiles(text)` -> a perceived `molfile.Mol` without a conformer.

Reference: utils/inference_utils.py:228 and :349 (`MolFromSmiles`), dock.py:27 (the default `--ligand_description`).  The reference
hands the string to rdkit; this is a reader for the OpenSMILES subset drug-like ligands are written in (opensmiles.org, sections 3.1
- 3.9).  Atoms stand in the order they are written, bonds in the order they are completed (a ring-closure bond when its second digit
is read, from the closing atom to the opening one), so the atom order of the written poses is the order of the string.

What is read: the organic subset and bracket atoms (isotope and atom class are read and dropped), the bond symbols - = # : / \\,
branches, ring closures 1-9 and %nn, aromatic (lower-case) atoms, @ / @@ and / \\.  Aromatic input is kekulised by a maximum matching
over the aromatic atoms that can take a double bond; `molfile.perceive` then decides aromaticity by its own model, exactly as it does
for a Kekule SDF, and assigns the hydrogen counts by its default-valence rule.  A bracket atom whose written hydrogen count disagrees
with that rule is a radical or a non-standard valence and is refused.

What is refused (ValueError naming the character position): unbalanced parentheses, an unclosed ring bond, an unknown symbol, `*`,
`$`, the extended chirality classes (@TH1, @AL1, @SP1, @TB1, @OH1 ...), `.`, an empty string, aromatic atoms that cannot be kekulised.
A ring bond's symbol stands on the opening digit, or on both digits; a symbol on the closing digit alone contradicts the opening digit
(which was written without one) and is refused with the other contradictions -- stricter than OpenSMILES, which lets it stand there.

Not here: hydrogens are not added, nothing is canonicalised, there is no SMILES writer.

Stereo.  `@` / `@@` become `Atom.chiral_tag` in the convention `perceive` uses for a 3-D pose: with the neighbours in the molecule's
bond order (an implicit hydrogen last), a positive volume of the first three neighbour vectors is CHI_TETRAHEDRAL_CCW.  `@` lists the
neighbours counter-clockwise seen from the first one IN WRITTEN ORDER (an implicit hydrogen right after the atom, ring-closure digits
where they stand); written order and bond order differ by a permutation, whose parity corrects the tag.  A tag on an atom that fails
`molfile.is_stereocentre` is dropped.  `/` and `\\` become `mol.double_bond_stereo`: (a, b, c, d, "cis" | "trans") for the flagged
substituents a and d of the double bond b=c.
"""
from __future__ import annotations

from .molfile import Atom, Bond, Mol, SYMBOLS, _default_valences, _rule_hydrogens, _symmetry_classes, is_stereocentre, perceive

_Z = {s: i + 1 for i, s in enumerate(SYMBOLS)}
_ORGANIC = ("Cl", "Br", "B", "C", "N", "O", "P", "S", "F", "I")
_AROMATIC = {"b": "B", "c": "C", "n": "N", "o": "O", "p": "P", "s": "S", "se": "Se", "as": "As"}
_BOND_TYPE = {"-": 1, "=": 2, "#": 3, ":": 4, "/": 1, "\\": 1}
_CHIRAL_CLASSES = ("TH", "AL", "SP", "TB", "OH")


def _fail(pos, what):
    raise ValueError(f"SMILES, position {pos}: {what}")


def _parse(s, off):
    """-> atoms (dicts), bonds ([a, b, type, default?, direction]) of the string s; `off` is added to reported positions."""
    atoms, bonds, stack, rings = [], [], [], {}
    prev, pending, n_ring, i = None, None, 0, 0

    def link(a, b, sym, frm, pos):
        if a == b or any({x[0], x[1]} == {a, b} for x in bonds):
            _fail(pos, "a second bond between the same two atoms")
        both = atoms[a]["aromatic"] and atoms[b]["aromatic"]
        t = _BOND_TYPE[sym] if sym else (4 if both else 1)
        bonds.append([a, b, t, sym is None, (sym, frm) if sym in ("/", "\\") else None])

    def add_atom(z, symbol, aromatic, pos, bracket=False, hcount=0, charge=0, chir=None):
        nonlocal prev, pending
        idx = len(atoms)
        atoms.append({"z": z, "symbol": symbol, "aromatic": aromatic, "pos": pos, "bracket": bracket, "hcount": hcount, "charge": charge,
                      "chir": chir, "order": []})
        if prev is not None:
            link(prev, idx, pending[0] if pending else None, prev, pos)
            atoms[prev]["order"].append(("a", idx))
            atoms[idx]["order"].append(("a", prev))
        elif pending:
            _fail(pending[1] + off, "a bond symbol in front of the first atom")
        atoms[idx]["order"] += [("h",)] * hcount
        prev, pending = idx, None

    while i < len(s):
        ch = s[i]
        if ch in _BOND_TYPE:
            if pending or prev is None:
                _fail(i + off, f"bond symbol {ch!r} without an atom in front of it")
            pending = (ch, i)
            i += 1
        elif ch == "(":
            if prev is None or pending:
                _fail(i + off, "a branch must follow an atom")
            if i + 1 < len(s) and s[i + 1] == ")":
                _fail(i + off, "an empty branch")
            stack.append((prev, i))
            i += 1
        elif ch == ")":
            if not stack or pending:
                _fail(i + off, "unbalanced parentheses" if not stack else "a bond symbol in front of ')'")
            prev = stack.pop()[0]
            i += 1
        elif ch.isdigit() or ch == "%":
            start = i
            if ch == "%":
                if not (s[i + 1:i + 3].isdigit() and len(s[i + 1:i + 3]) == 2):
                    _fail(i + off, "'%' must be followed by two digits")
                key, i = int(s[i + 1:i + 3]), i + 3
            else:
                key, i = int(ch), i + 1
            if prev is None:
                _fail(start + off, "a ring-closure digit without an atom in front of it")
            sym = pending[0] if pending else None
            pending = None
            if key not in rings:
                rings[key] = (prev, sym, start, n_ring)
                atoms[prev]["order"].append(("r", n_ring))
                n_ring += 1
                continue
            a0, sym0, _, token = rings.pop(key)
            if sym is not None:
                flip = {"/": "\\", "\\": "/"}
                if sym0 is None or (flip.get(sym0, sym0) != sym):
                    _fail(start + off, f"ring bond {key} is written {sym0 or 'without a symbol'} where it opens and {sym} where it closes")
            link(prev, a0, sym0, a0, start + off)
            atoms[a0]["order"][atoms[a0]["order"].index(("r", token))] = ("a", prev)
            atoms[prev]["order"].append(("a", a0))
        elif ch == "[":
            end = s.find("]", i)
            if end < 0:
                _fail(i + off, "'[' without ']'")
            j = i + 1
            while s[j].isdigit():                                   # isotope: read and dropped
                j += 1
            if s[j] == "*":
                _fail(j + off, "the wildcard atom '*' is not supported")
            if s[j:j + 2] in _AROMATIC or s[j] in _AROMATIC:
                sym = s[j:j + 2] if s[j:j + 2] in _AROMATIC else s[j]
                symbol, aromatic = _AROMATIC[sym], True
            elif s[j:j + 2] in _Z and s[j:j + 2][1:].islower():
                sym, aromatic = s[j:j + 2], False
                symbol = sym
            elif s[j] in _Z:
                sym, aromatic = s[j], False
                symbol = sym
            else:
                _fail(j + off, f"unknown element symbol at {s[j:j + 2]!r}")
            j += len(sym)
            chir = None
            if s[j] == "@":
                chir, j = "@", j + 1
                if s[j] == "@":
                    chir, j = "@@", j + 1
                elif s[j:j + 2] in _CHIRAL_CLASSES and s[j:j + 2] != "OH" or (s[j:j + 2] == "OH" and s[j + 2].isdigit()):
                    _fail(j + off, f"chirality class @{s[j:j + 2]} is not supported (only @ and @@)")
            hcount = 0
            if s[j] == "H":
                hcount, j = 1, j + 1
                if s[j].isdigit():
                    hcount, j = int(s[j]), j + 1
            charge = 0
            if s[j] in "+-":
                sign = 1 if s[j] == "+" else -1
                k = j
                while s[k] == s[j]:
                    k += 1
                charge, j = sign * (k - j), k
                if charge in (1, -1) and s[j].isdigit():
                    k = j
                    while s[k].isdigit():
                        k += 1
                    charge, j = sign * int(s[j:k]), k
            if s[j] == ":":                                         # atom class: read and dropped
                j += 1
                if not s[j].isdigit():
                    _fail(j + off, "an atom class must be a number")
                while s[j].isdigit():
                    j += 1
            if j != end:
                _fail(j + off, f"unexpected {s[j]!r} inside a bracket atom")
            add_atom(_Z[symbol], symbol, aromatic, i + off, True, hcount, charge, chir)
            i = end + 1
        elif ch == ".":
            _fail(i + off, "'.': molecules of several components are not supported")
        elif ch == "*":
            _fail(i + off, "the wildcard atom '*' is not supported")
        elif ch == "$":
            _fail(i + off, "quadruple bonds ('$') are not supported")
        else:
            sym = next((o for o in _ORGANIC if s.startswith(o, i)), None)
            if sym is not None:
                add_atom(_Z[sym], sym, False, i + off)
            elif ch in ("b", "c", "n", "o", "p", "s"):
                sym = ch
                add_atom(_Z[_AROMATIC[ch]], _AROMATIC[ch], True, i + off)
            else:
                _fail(i + off, f"unknown symbol {ch!r}")
            i += len(sym)
    if pending:
        _fail(pending[1] + off, "a bond symbol at the end of the string")
    if stack:
        _fail(stack[-1][1] + off, "unbalanced parentheses: this '(' is never closed")
    if rings:
        key, (_, _, pos, _) = sorted(rings.items(), key=lambda kv: kv[1][2])[0]
        _fail(pos + off, f"ring bond {key} is never closed")
    if not atoms:
        _fail(off, "an empty string")
    return atoms, bonds


def _kekulise(atoms, bonds):
    """Turns every aromatic (type 4) bond into a single or double one, in place.  A bond written without a symbol between two
    aromatic atoms is aromatic only inside a ring (the bond between the rings of biphenyl is single).  The aromatic atoms that can
    take a double bond -- those whose bonds (aromatic ones counted once) and written hydrogens stay below the smallest default valence
    that covers them: c, a two-connected n, [n+]; not [nH], a three-connected n, o, s -- must ALL find a partner: a maximum matching
    over them along the aromatic bonds, refused when it is not perfect."""
    import networkx as nx
    if not any(b[2] == 4 for b in bonds):
        if any(a["aromatic"] for a in atoms):
            _fail(next(a["pos"] for a in atoms if a["aromatic"]), "an aromatic atom outside any ring cannot be kekulised")
        return
    g = nx.Graph()
    g.add_nodes_from(range(len(atoms)))
    g.add_edges_from((b[0], b[1]) for b in bonds)
    bridges = set(frozenset(e) for e in nx.bridges(g))
    for b in bonds:
        if b[2] == 4 and b[3] and frozenset((b[0], b[1])) in bridges:
            b[2] = 1
    total = [0] * len(atoms)
    for b in bonds:
        w = 1 if b[2] == 4 else b[2]
        total[b[0]] += w
        total[b[1]] += w
    cand = []
    for i, a in enumerate(atoms):
        if not a["aromatic"]:
            continue
        need = total[i] + (a["hcount"] if a["bracket"] else 0)
        fit = [v for v in _default_valences(a["z"], a["charge"]) if v >= need]
        if fit and fit[0] > need:
            cand.append(i)
    m = nx.Graph()
    m.add_nodes_from(cand)
    in_cand = set(cand)
    m.add_edges_from((b[0], b[1]) for b in bonds if b[2] == 4 and b[0] in in_cand and b[1] in in_cand)
    match = nx.max_weight_matching(m, maxcardinality=True)
    paired = set(x for e in match for x in e)
    if len(paired) != len(cand):
        left = min(in_cand - paired)
        _fail(atoms[left]["pos"], f"the aromatic atoms cannot be kekulised (no double bond for this {atoms[left]['symbol']})")
    double = set(frozenset(e) for e in match)
    for b in bonds:
        if b[2] == 4:
            b[2] = 2 if frozenset((b[0], b[1])) in double else 1


def _parity(written, reference):
    perm = [reference.index(w) for w in written]
    return sum(1 for x in range(len(perm)) for y in range(x + 1, len(perm)) if perm[x] > perm[y]) % 2


def mol_from_smiles(text) -> Mol:
    """A perceived `molfile.Mol` without a conformer (`pos` empty) from a SMILES string; see the module text for what is read, what is
    refused (ValueError with the character position) and how stereo is stored.  `lig_atom_featurizer`, `get_lig_graph`,
    `get_transformation_mask` and `conformer_embedding.distance_bounds` take it as they take a molecule read from a file."""
    if not isinstance(text, str):
        raise ValueError(f"SMILES, position 0: not a string ({text!r})")
    s = text.strip()
    off = len(text) - len(text.lstrip())
    recs, bonds = _parse(s, off)
    _kekulise(recs, bonds)
    atoms = [Atom(i, a["z"], a["symbol"], a["charge"]) for i, a in enumerate(recs)]
    mol = Mol(atoms, [Bond(b[0], b[1], b[2]) for b in bonds], [], name=s)
    for i, a in enumerate(recs):
        if a["bracket"] and _rule_hydrogens(mol, i) != a["hcount"]:
            _fail(a["pos"], f"[{a['symbol']}] is written with {a['hcount']} hydrogen(s) where the default valence gives "
                            f"{_rule_hydrogens(mol, i)}: radicals and non-standard valences are not supported")
    perceive(mol)
    # ---- tetrahedral tags: written order -> bond order
    cls = None
    for i, a in enumerate(recs):
        if a["chir"] is None:
            continue
        if cls is None:
            cls = _symmetry_classes(mol)
        if not is_stereocentre(mol, i, cls):
            continue
        reference = [("a", j) for j, _ in mol.neighbors(i)] + [("h",)] * mol.atoms[i].num_hs
        if sorted(reference) != sorted(a["order"]):
            continue
        ccw = (a["chir"] == "@") == (_parity(a["order"], reference) == 0)
        mol.atoms[i].chiral_tag = "CHI_TETRAHEDRAL_CCW" if ccw else "CHI_TETRAHEDRAL_CW"
    # ---- double bonds: the side of the first flagged substituent of either end
    for k, b in enumerate(bonds):
        if mol.bonds[k].type != 2:
            continue
        ends = []
        for x in (b[0], b[1]):
            for j, kk in mol.neighbors(x):
                d = bonds[kk][4]
                if kk != k and d is not None:
                    sym, frm = d
                    ends.append((j, (sym == "/") == (frm == x)))        # True: the substituent lies "above" the double-bond atom
                    break
        if len(ends) == 2:
            mol.double_bond_stereo.append((ends[0][0], b[0], b[1], ends[1][0], "cis" if ends[0][1] == ends[1][1] else "trans"))
    return mol
