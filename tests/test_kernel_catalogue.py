"""The kernel catalogue (ba_launch.h): which alignment kernels the library holds. Every kernel translation unit registers its
families while the library loads; the host looks a batch's kernel up there and fails with a message when it is missing. The set
below is written out by hand -- it is what the hand-written launcher tables held before the catalogue replaced them -- so a
condition in ba_kernels.hip that drifts from what batch_build assumes shows up here, without a GPU: nothing is launched."""
import ctypes as C
import itertools

FAMILIES = ("pair", "tiled", "multi", "multi256", "multi512", "multi_g2", "multi_g3", "small", "quad")   # ba::KernelFamily, in order
KINDS = range(4)            # AA, NUC, BYTES, PROFILE
CLASSES = range(6)          # 128 << c cells for c = 0 .. 4 (1, 2, 4, 8, 16 packed registers per lane); 5 = row-tiled
TILED = 5


def expected():
    """(family, kind, class, special) -> forms"""
    e = {}
    for special in (0, 1):
        for kind in KINDS:
            for pc in range(5):
                e["pair", kind, pc, special] = 1            # 4 kinds x classes {1, 2, 4, 8, 16}, plain and special
            e["tiled", kind, TILED, special] = 1            # 4 row-tiled, plain and special
    for kind in (0, 1, 2):
        for pc in range(5):
            e["multi", kind, pc, 0] = 1                     # k_multi: the sequence kinds x 5 classes ...
            e["multi", kind, pc, 1] = 2                     # ... special: LOCAL_START and FREE_QUERY_START_GAPS forms
    for pc in (2, 3, 4):
        e["multi256", 1, pc, 0] = 1                         # 256-cell slots: DNA, classes {4, 8, 16}
    for pc in (3, 4):
        e["multi512", 1, pc, 0] = 1                         # 512-cell slots: DNA, classes {8, 16}
    for pc in (2, 3):
        e["multi_g2", 1, pc, 0] = 1                         # the four-wave geometries: DNA, classes {4, 8}
        e["multi_g3", 1, pc, 0] = 1
    for kind in KINDS:
        for pc in range(4):
            e["small", kind, pc, 0] = 1                     # k_small: 4 kinds x classes {1, 2, 4, 8} ...
            if kind != 3:
                e["small", kind, pc, 1] = 2                 # ... special: the sequence kinds, both forms
        e["quad", kind, 0, 0] = 1                           # k_quad: one per kind
    return e


def forms(hip, family, kind, pc, special):
    f = hip.lib().ba_dev_kernel_forms
    f.argtypes = [C.c_int] * 4
    f.restype = C.c_int
    return f(FAMILIES.index(family) if isinstance(family, str) else family, kind, pc, special)


def test_expected_list_has_the_size_of_the_old_tables():
    e = expected()
    count = lambda fam: sum(1 for k in e if k[0] == fam)
    assert [count(f) for f in FAMILIES] == [40, 8, 30, 3, 2, 2, 2, 28, 4]


def test_catalogue_holds_exactly_the_expected_kernels(devlib):
    e = expected()
    got = {}
    for fam, kind, pc, special in itertools.product(FAMILIES, KINDS, CLASSES, (0, 1)):
        n = forms(devlib, fam, kind, pc, special)
        if n:
            got[fam, kind, pc, special] = n
    assert sorted(set(e) - set(got)) == [], "kernels the host may ask for are missing"
    assert sorted(set(got) - set(e)) == [], "kernels nobody listed"
    assert got == e


def test_absent_combinations_are_reported_not_called(devlib):
    for fam, kind, pc, special in (("multi256", 1, 1, 0), ("small", 0, 4, 0), ("multi", 3, 2, 0), ("multi", 3, 2, 1), ("small", 3, 0, 1),
                                   ("multi_g2", 1, 4, 0), ("multi_g3", 0, 2, 0), ("multi512", 1, 2, 0), ("quad", 0, 1, 0), ("quad", 0, 0, 1),
                                   ("pair", 0, TILED, 0), ("tiled", 0, 4, 0), ("multi256", 1, 2, 1)):
        assert forms(devlib, fam, kind, pc, special) == 0, (fam, kind, pc, special)
    # out of range in every argument: absent, not an index past a table
    for args in ((-1, 0, 0, 0), (len(FAMILIES), 0, 0, 0), (0, -1, 0, 0), (0, 4, 0, 0), (0, 0, -1, 0), (0, 0, 6, 0), (0, 0, 0, 2), (0, 0, 0, -1)):
        assert forms(devlib, *args) == 0, args


def test_release_library_does_not_export_the_query(hip):
    assert hip.lib().ba_dev_build() == 0
    assert not hasattr(hip.lib(), "ba_dev_kernel_forms")
