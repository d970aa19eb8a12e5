"""rust/ -- the `simd_hip` feature for the reference crate -- is source nobody here can compile (no rustc / cargo in the image), and the
crate's own sources are not part of this repository. What can be checked from the repository alone is checked here:
  * the patches for scan_block.rs, scores.rs and cigar.rs only add lines (well-formed hunks, no line removed), and lib.rs.patch removes
    nothing but the five cfg gates it widens;
  * in the HIP sources of rust/src, no item that survives the cfg gates of a build with only `simd_hip` mentions the SIMD layer (Simd,
    HalfSimd, LutSimd, TraceType, the simd_* / halfsimd_* intrinsics wrappers, the lane count L): a small cfg-aware scanner removes what
    `#[cfg(not(feature = "simd_hip"))]`, the CPU feature gates and `#[cfg(test)]` compile out and greps the rest;
  * the FFI block of src/hip.rs declares only functions that include/block_aligner_hip.h declares.
"""
import os
import re

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
RUST = os.path.join(ROOT, "rust")
PATCHES = ["Cargo.toml.patch", "cigar.rs.patch", "lib.rs.patch", "scan_block.rs.patch", "scores.rs.patch"]

CPU_FEATURES = ("simd_sse2", "simd_avx2", "simd_wasm", "simd_neon")
SIMD_WORDS = re.compile(r"\b(Simd|HalfSimd|LutSimd|TraceType|L|simd_[a-z0-9_]+|halfsimd_[a-z0-9_]+|lutsimd_[a-z0-9_]+)\b")


def strip_comments(text):
    text = re.sub(r"//[^\n]*", "", text)
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def cfg_enabled(expr):
    """Value of a cfg predicate in a build with ONLY the simd_hip feature (and not under test)."""
    expr = expr.strip()
    m = re.fullmatch(r'feature\s*=\s*"([a-z0-9_]+)"', expr)
    if m:
        return m.group(1) == "simd_hip"
    if expr == "test":
        return False
    if expr.startswith("target_arch"):
        return True   # (irrelevant to the question asked here)
    for op in ("not", "any", "all"):
        if expr.startswith(op + "(") and expr.endswith(")"):
            inner, parts, depth, cur = expr[len(op) + 1:-1], [], 0, ""
            for ch in inner:
                if ch == "," and depth == 0:
                    parts.append(cur); cur = ""
                else:
                    depth += ch == "("; depth -= ch == ")"; cur += ch
            if cur.strip():
                parts.append(cur)
            vals = [cfg_enabled(p) for p in parts]
            return (not vals[0]) if op == "not" else (any(vals) if op == "any" else all(vals))
    raise AssertionError("cfg predicate not understood: " + expr)


def item_end(text, start):
    """Index just past the item that begins at `start` (after its attributes). The item's header ends with the first line that ends in
    `;` (no body), in `{` (the body's brace: const-generic arguments like `Block<{ TRACE }>` earlier in the header are not it) or in `}`
    (a one-line body)."""
    i = start
    while True:
        nl = text.find("\n", i)
        nl = len(text) if nl < 0 else nl
        line = text[i:nl].rstrip()
        if line.endswith(";") and line.count("{") == line.count("}"):
            return nl
        if line.endswith("{"):
            depth, k = 1, i + len(line)
            while depth:
                ch = text[k]
                depth += ch == "{"; depth -= ch == "}"
                k += 1
            return k
        if line.endswith("}") and "{" in line:
            return nl
        assert nl < len(text), "unterminated item"
        i = nl + 1


def surviving(text):
    """The source with every cfg-disabled item removed (a build with only `simd_hip`)."""
    text = strip_comments(text)
    out, i = [], 0
    attr = re.compile(r"#\[cfg\((.*)\)\]\s*$")
    lines = text.split("\n")
    pos = [0]
    for ln in lines:
        pos.append(pos[-1] + len(ln) + 1)
    k = 0
    keep_from = 0
    while k < len(lines):
        m = attr.match(lines[k].strip()) if lines[k].strip().startswith("#[cfg(") else None
        if m and not cfg_enabled(m.group(1)):
            # skip this attribute, any further attributes, then the item
            j = k + 1
            while j < len(lines) and (lines[j].strip().startswith("#[") or not lines[j].strip()):
                j += 1
            end = item_end(text, pos[j])
            out.append(text[keep_from:pos[k]])
            keep_from = end
            while k < len(lines) and pos[k + 1] <= end:
                k += 1
            if pos[k] < end:   # the item ended inside this line
                k += 1
            continue
        k += 1
    out.append(text[keep_from:])
    return "".join(out)


def hunks(name):
    """[(old_start, old_count, new_start, new_count, body lines)] of rust/<name>; asserts every hunk's body matches its header."""
    out, cur = [], None
    for line in open(os.path.join(RUST, name)).read().split("\n"):
        m = re.match(r"@@ -(\d+)(?:,(\d+))? \+(\d+)(?:,(\d+))? @@", line)
        if m:
            cur = (int(m.group(1)), int(m.group(2) or 1), int(m.group(3)), int(m.group(4) or 1), [])
            out.append(cur)
        elif cur is not None and line[:1] in (" ", "+", "-"):
            cur[4].append(line)
    for old_start, old_count, new_start, new_count, body in out:
        assert sum(l[0] != "+" for l in body) == old_count and sum(l[0] != "-" for l in body) == new_count, (name, old_start)
    return out


def test_the_cpu_build_is_unchanged_by_the_gates():
    """With a CPU feature and without simd_hip every original line is still there: the patches only add lines (and widen five cfg gates)."""
    assert sorted(f for f in os.listdir(RUST) if f.endswith(".patch")) == PATCHES
    for name in PATCHES:
        hs = hunks(name)
        assert hs, name
        removed = [l[1:] for h in hs for l in h[4] if l[0] == "-"]
        if name in ("scan_block.rs.patch", "scores.rs.patch", "cigar.rs.patch"):
            assert not removed, (name, removed)   # the original file is a subsequence of the patched one
        elif name == "lib.rs.patch":
            added = [l[1:] for h in hs for l in h[4] if l[0] == "+"]
            assert len(removed) == 5, removed
            for gate in removed:                  # every removed gate comes back with simd_hip among its features
                feats = set(re.findall(r'feature = "(\w+)"', gate))
                assert gate.startswith("#[cfg(") and any(set(re.findall(r'feature = "(\w+)"', g)) == feats | {"simd_hip"} for g in added), gate
    lib = "\n".join(l[1:] for h in hunks("lib.rs.patch") for l in h[4] if l[0] == "+")
    assert 'feature = "simd_hip"' in lib and "pub mod hip;" in lib
    assert "+simd_hip = []" in open(os.path.join(RUST, "Cargo.toml.patch")).read()
    assert any("fn set_runs" in l for h in hunks("cigar.rs.patch") for l in h[4] if l[0] == "+")


def test_no_simd_identifier_survives_in_the_hip_sources():
    for name in ("hip.rs", "scan_block_hip.rs"):
        code = surviving(open(os.path.join(RUST, "src", name)).read())
        code = re.sub(r'"(\\.|[^"\\])*"', '""', code)   # string literals (the feature names among them)
        hits = sorted({m.group(0) for m in SIMD_WORDS.finditer(code)})
        assert not hits, (name, hits)


def test_ffi_declarations_exist_in_the_header():
    hip_rs = strip_comments(open(os.path.join(RUST, "src", "hip.rs")).read())
    block = hip_rs[hip_rs.index('extern "C" {'):]
    block = block[:block.index("\n}\n")]
    fns = re.findall(r"pub fn (\w+)\(", block)
    assert len(fns) > 50
    header = open(os.path.join(ROOT, "include", "block_aligner_hip.h")).read()
    missing = [f for f in fns if not re.search(r"\b%s\s*\(" % f, header)]
    assert not missing, missing
    ex = open(os.path.join(RUST, "examples", "dump_golden.rs")).read()
    assert "Block::<TRACE, X_DROP, LOCAL_START, FQS, FQE>::new" in ex and "crate_golden_input.tsv" in ex
