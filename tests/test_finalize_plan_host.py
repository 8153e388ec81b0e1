"""The finalize's decisions and its key codec without a GPU: particle-sfm_amd/csrc/psfm_finalize_plan.h -- the form plan
psfm_fin_form() (key width, sort bits, own sort or rocPRIM, passes, which half the records start in, group plan or decode + scan),
the codec every finalize kernel reads its keys through, and the shard accounting of the per-frame path -- compiled for the host
through tests/host/shim and driven by tests/host/finalize_plan_host.cpp.  The plan is pinned at the shapes the project documents
(each expected value worked out here from the rule) and against a restatement of the rules over a sweep that crosses every
threshold by +-1; the codec over every key of small sequences and over the edge of the 32-bit format's domain."""
import ctypes
import itertools
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLAN_MAX_GROUPS = 16384       # groups the one-block plan kernel holds in LDS
SORT64_MAX_N = 5_000_000      # 64-bit keys: the own sort up to here
FIELDS = ("use32", "ok", "seq_bits", "seq_shift", "end_bit", "sort_form", "passes", "first_half", "ng", "offsets_form")


@pytest.fixture(scope="module")
def fin(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("fin_plan") / "libfin_plan_host.so")
    cmd = ["g++", "-O2", "-mfma", "-shared", "-fPIC", "-std=c++17", "-ffp-contract=off", "-I", os.path.join(ROOT, "tests", "host", "shim"), "-I", os.path.join(ROOT, "particle-sfm_amd", "csrc"),
           os.path.join(ROOT, "tests", "host", "finalize_plan_host.cpp"), "-o", out]
    subprocess.run(cmd, check=True)
    L = ctypes.CDLL(out)
    i32, i64, u64, vp = ctypes.c_int, ctypes.c_longlong, ctypes.c_ulonglong, ctypes.c_void_p
    L.psfm_host_fin_form.argtypes = [i32, i32, i32, i32, i64, i32, i32, i32, vp]
    L.psfm_host_fin_form.restype = None
    L.psfm_host_shard_offsets.argtypes = [vp, i32, vp, vp, vp]
    L.psfm_host_codec_sweep.argtypes = [i32, i32, i32, i32, vp, vp]
    L.psfm_host_codec_sweep.restype = i64
    L.psfm_host_tri_invert.argtypes = [ctypes.c_uint, vp, vp]
    L.psfm_host_tri_invert.restype = None
    L.psfm_host_batch_roundtrip.argtypes = [u64, i32, i32, i32, i32, i32, vp, vp]
    L.psfm_host_batch_roundtrip.restype = u64
    L.psfm_host_key32.argtypes = [u64, i32, i32]
    L.psfm_host_key32.restype = ctypes.c_uint
    return L


def bits_for(count):
    """The smallest b >= 1 with 2^b >= count."""
    b = 1
    while (1 << b) < count:
        b += 1
    return b


def shifts(G, n_flows):
    """psfm_track_dims: the grid index takes shift_b bits, birth and last bits_for(n_flows + 2) each."""
    shift_b = bits_for(G)
    return shift_b, shift_b + bits_for(n_flows + 2)


def grid(h, w, r):
    return ((h + r - 1) // r) * ((w + r - 1) // r)


def form(L, G, n_flows, n, n_seq=1, sort=1, plan=1, allowed=1):
    sb, sd = shifts(G, n_flows)
    out = (ctypes.c_longlong * 10)()
    L.psfm_host_fin_form(sb, sd, n_flows, n_seq, n, sort, plan, allowed, ctypes.addressof(out))
    return dict(zip(FIELDS, [int(v) for v in out]))


def restated(G, n_flows, n, n_seq, sort, plan, allowed):
    """The plan from its rules.  Groups: (last, birth) pairs with birth <= last <= n_flows + 1, numbered last (last + 1) / 2 + birth.
    32-bit keys hold group : grid index, with a batch's sequence number in front, when all of it fits 32 bits; else 64-bit keys
    last : birth : grid index.  The own sort: 8-bit digits, below 2^31 records, 64-bit keys only up to SORT64_MAX_N records unless
    forced; it ends in the first half, so the records start there when its pass count is even; rocPRIM sorts second -> first half.
    The group plan: single sequences, at most PLAN_MAX_GROUPS groups, below 2^31 records."""
    sb, sd = shifts(G, n_flows)
    lmax = n_flows + 1
    ng = (lmax + 1) * (lmax + 2) // 2
    seq_bits = 0 if n_seq <= 1 else (n_seq - 1).bit_length()
    key32 = sb + (1 if ng <= 2 else (ng - 1).bit_length())
    use32 = key32 + seq_bits <= 32
    seq_shift = key32 if use32 else sd + (sd - sb)
    end_bit = seq_shift + seq_bits
    own = sort != 0 and n < 2**31 and (use32 or sort == 2 or n <= SORT64_MAX_N)
    passes = -(-end_bit // 8)
    return dict(use32=int(use32), ok=int(end_bit <= 64), seq_bits=seq_bits, seq_shift=seq_shift, end_bit=end_bit,
                sort_form=(1 if use32 else 2) if own else 3, passes=passes, first_half=int(own and passes % 2 == 0), ng=ng,
                offsets_form=1 if (allowed and plan and ng <= PLAN_MAX_GROUPS and n < 2**31) else 3)


def test_plan_at_the_headline_shape(fin):
    G = grid(1080, 1920, 2)
    assert G == 540 * 960 and shifts(G, 100)[0] == 19            # 2^19 = 524288 >= 518400 > 2^18
    ng = 101 * 102 // 2 + 101 + 1                                # last <= 101: pairs below last = 101, its 102 births
    assert ng == 5253 and 2**12 < ng <= 2**13                    # 13 group bits
    f = form(fin, G, 100, 2_000_000)
    assert f == dict(use32=1, ok=1, seq_bits=0, seq_shift=19 + 13, end_bit=32, sort_form=1, passes=4, first_half=1, ng=5253, offsets_form=1)


@pytest.mark.parametrize("n_flows,ng,offsets_form", [(178, 16290, 1), (179, 16471, 3), (400, None, 3)])
def test_plan_switches_to_decode_and_scan_where_the_groups_leave_lds(fin, n_flows, ng, offsets_form):
    f = form(fin, grid(24, 30, 2), n_flows, 50_000)
    lmax = n_flows + 1
    assert f["ng"] == (lmax + 1) * (lmax + 2) // 2               # pairs birth <= last <= lmax
    if ng is not None:
        assert f["ng"] == ng
    assert (f["ng"] <= PLAN_MAX_GROUPS) == (offsets_form == 1)
    assert f["offsets_form"] == offsets_form


def test_plan_key_width_at_its_switch(fin):
    G = grid(64, 90, 1)
    assert shifts(G, 1021)[0] == 13                              # 5760 grid points
    # 1021 flows: 1023 * 1024 / 2 = 523776 groups <= 2^19 -> 13 + 19 = 32 bits; 1022 flows: 524800 groups need 20
    f, g = form(fin, G, 1021, 100_000), form(fin, G, 1022, 100_000)
    assert (f["ng"], g["ng"]) == (523776, 524800)
    assert f["use32"] == 1 and f["end_bit"] == 32 and f["sort_form"] == 1 and f["first_half"] == 1
    assert g["use32"] == 0 and g["sort_form"] == 2 and g["end_bit"] == 13 + 2 * 10 and g["passes"] == 5 and g["first_half"] == 0


def test_plan_of_long_sequences_on_64_bit_keys(fin):
    f = form(fin, grid(1080, 1920, 2), 400, 3_000_000)           # 19 + 2 * 9 (402 times need 9 bits)
    assert f["use32"] == 0 and f["end_bit"] == f["seq_shift"] == 37 and f["passes"] == 5 and f["sort_form"] == 2
    assert f["first_half"] == 0 and f["offsets_form"] == 3       # five passes end in the first half from the second
    f = form(fin, grid(480, 640, 1), 999, 3_000_000)             # 307200 grid points: 19 bits; 1001 times: 10
    assert f["use32"] == 0 and f["end_bit"] == 19 + 2 * 10 == 39


def test_plan_sort_by_record_count_and_switches(fin):
    G = grid(1080, 1920, 2)
    assert [form(fin, G, 400, n)["sort_form"] for n in (SORT64_MAX_N, SORT64_MAX_N + 1, 2**31)] == [2, 3, 3]
    assert [form(fin, G, 100, n)["sort_form"] for n in (SORT64_MAX_N + 1, 2**31 - 1, 2**31)] == [1, 1, 3]
    assert form(fin, G, 100, 2**31)["offsets_form"] == 3 and form(fin, G, 100, 2**31 - 1)["offsets_form"] == 1
    for nf in (100, 400):                                        # PSFM_FIN_SORT=0 PSFM_FIN_PLAN=0: rocPRIM, decode + scan, second half
        f = form(fin, G, nf, 1000, sort=0, plan=0)
        assert (f["sort_form"], f["offsets_form"], f["first_half"]) == (3, 3, 0)
    # PSFM_FIN_SORT=2: the own sort at any n < 2^31
    assert [form(fin, G, 400, n, sort=2)["sort_form"] for n in (SORT64_MAX_N + 1, 2**31 - 1, 2**31)] == [2, 2, 3]
    assert [form(fin, G, 100, n, sort=2)["sort_form"] for n in (2**31 - 1, 2**31)] == [1, 3]


def test_plan_of_a_batch(fin):
    G = grid(48, 64, 1)
    assert shifts(G, 178)[0] == 12
    f = form(fin, G, 178, 400_000, n_seq=32, allowed=0)          # 12 + 14 (16290 groups) + 5 sequence bits = 31
    assert f == dict(use32=1, ok=1, seq_bits=5, seq_shift=26, end_bit=31, sort_form=1, passes=4, first_half=1, ng=16290, offsets_form=3)
    f = form(fin, G, 180, 400_000, n_seq=33, allowed=0)          # 12 + 15 (16653 groups) + 6 > 32: 64-bit keys, 12 + 2 * 8 bits
    assert f["ng"] == 16653 and f["use32"] == 0 and f["seq_bits"] == 6 and f["seq_shift"] == 28 and f["end_bit"] == 34
    assert f["sort_form"] == 2 and f["passes"] == 5 and f["first_half"] == 0 and f["offsets_form"] == 3 and f["ok"] == 1
    f = form(fin, grid(1080, 1920, 2), 100, 2_000_000, n_seq=1, allowed=0)      # a batch of one whose key fills the word
    assert f["use32"] == 1 and f["seq_bits"] == 0 and f["seq_shift"] == 32 and f["end_bit"] == 32 and f["offsets_form"] == 3
    # a key that does not fit 64 bits beside the sequence number: 31 + 2 * 16 = 63 bits, one sequence bit fits, two do not
    assert [form(fin, 2**31, 65000, 10, n_seq=k, allowed=0)["ok"] for k in (1, 2, 3)] == [1, 1, 0]


def test_plan_equals_its_restatement_across_every_threshold(fin):
    Gs = [1, 2, 3, 180, 3072, 4095, 4096, 4097, 5760, 8191, 8192, 8193, 2**18, 2**18 + 1, 518400, 2**19, 2**19 + 1, 2**24]
    flows = [1, 2, 3, 6, 7, 100, 101, 126, 127, 177, 178, 179, 180, 254, 255, 361, 362, 400, 510, 511, 1021, 1022, 1023, 4000]
    seqs = [1, 2, 3, 4, 5, 31, 32, 33, 64]
    ns = [1, SORT64_MAX_N - 1, SORT64_MAX_N, SORT64_MAX_N + 1, 2**31 - 1, 2**31, 2**31 + 1]
    switches = [(1, 1, 1), (1, 1, 0), (0, 0, 1), (0, 1, 1), (2, 1, 1), (2, 0, 0), (1, 0, 1)]
    seen = set()
    for G, nf, n_seq in itertools.product(Gs, flows, seqs):
        for k, n in enumerate(ns):
            sort, plan, allowed = switches[(k + nf + n_seq) % len(switches)]
            if n_seq > 1:
                allowed = 0
            got, want = form(fin, G, nf, n, n_seq, sort, plan, allowed), restated(G, nf, n, n_seq, sort, plan, allowed)
            assert got == want, (G, nf, n_seq, n, sort, plan, allowed)
            seen.add((got["use32"], got["sort_form"], got["first_half"], got["offsets_form"], got["seq_bits"] > 0))
    # the sweep met every form in both key widths, both halves, with and without sequence bits
    assert {(u, s) for u, s, _, _, _ in seen} == {(1, 1), (1, 3), (0, 2), (0, 3)}
    assert {(h, o) for _, _, h, o, _ in seen} == {(0, 1), (0, 3), (1, 1), (1, 3)}


@pytest.mark.parametrize("lmax", [1, 2, 101, 179, 1022])
def test_codec_round_trips_every_key_of_small_sequences(fin, lmax):
    """pack -> psfm_key32 -> psfm_key_fields gives (last, birth, idx) back, in the 64-bit format too, and both formats name the same
    group: every last <= lmax, every birth <= last, at the narrowest grid index and at the widest the 32-bit format leaves room for."""
    tri_bits = bits_for((lmax + 1) * (lmax + 2) // 2)
    for shift_b in (1, 32 - tri_bits):
        shift_d = shift_b + bits_for(lmax + 1)                   # n_flows = lmax - 1
        bad, tried = (ctypes.c_int * 3)(-1, -1, -1), ctypes.c_longlong(0)
        fails = fin.psfm_host_codec_sweep(lmax, shift_b, shift_d, 0, ctypes.addressof(bad), ctypes.addressof(tried))
        assert tried.value == 4 * (lmax + 1) * (lmax + 2) // 2
        assert fails == 0, "first failing (last, birth, idx) = %s at shift_b %d" % (list(bad), shift_b)


def test_codec_at_the_edge_of_the_32_bit_domain(fin):
    """shift_b >= 1 and group bits + shift_b <= 32 leave last <= 65534 (65534 * 65537 < 2^32 < 65535 * 65538): for every last up to
    there, birth in {0, 1, last - 1, last} -- the inversion's estimate and its correction loops at both ends of every row, up to the
    largest group number a key can carry -- come back exactly."""
    lmax = 65534
    assert lmax * (lmax + 3) < 2**32 <= (lmax + 1) * (lmax + 4)
    assert bits_for((lmax + 1) * (lmax + 2) // 2) == 31          # 31 + shift_b = 1: the word is full
    bad, tried = (ctypes.c_int * 3)(-1, -1, -1), ctypes.c_longlong(0)
    fails = fin.psfm_host_codec_sweep(lmax, 1, 1 + bits_for(lmax + 1), 1, ctypes.addressof(bad), ctypes.addressof(tried))
    assert tried.value == 16 * (lmax + 1)
    assert fails == 0, "first failing (last, birth, idx) = %s" % list(bad)
    last, birth = ctypes.c_int(-1), ctypes.c_int(-1)
    top = lmax * (lmax + 1) // 2 + lmax                          # (last, birth) = (65534, 65534)
    for tri, want in ((top, (lmax, lmax)), (top - lmax, (lmax, 0)), (top - lmax - 1, (lmax - 1, lmax - 1)), (0, (0, 0)), (1, (1, 0)), (2, (1, 1))):
        fin.psfm_host_tri_invert(tri, ctypes.addressof(last), ctypes.addressof(birth))
        assert (last.value, birth.value) == want, tri


@pytest.mark.parametrize("use32,seq_shift,seq", [(1, 26, 31), (1, 31, 1), (1, 32, 0), (0, 28, 32), (0, 32, 5), (0, 37, 63), (0, 63, 1)])
def test_batch_keys_split_back_into_sequence_and_key(fin, use32, seq_shift, seq):
    """(sequence << seq_shift | key) for seq_shift below, at and above 32: a 32-bit word with seq_shift 32 is a batch of ONE sequence
    whose key fills the word -- nothing to write, sequence 0 to read."""
    shift_b = 12
    key_bits = seq_shift - shift_b if use32 else (seq_shift - shift_b) // 2      # group bits / bits of last and of birth
    shift_d = shift_b + ((seq_shift - shift_b) // 2 if not use32 else 9)
    for last, birth, idx in ((0, 0, 0), (3, 2, 4095), (5, 5, 1), (200, 17, 2730)):
        if use32 and (last * (last + 1) // 2 + birth) >> key_bits:
            continue
        if not use32 and last >> key_bits:
            continue
        k = (last << shift_d) | (birth << shift_b) | idx
        own = fin.psfm_host_key32(k, shift_b, shift_d) if use32 else k
        stored, seq_out = ctypes.c_ulonglong(0), ctypes.c_int(-1)
        back = fin.psfm_host_batch_roundtrip(k, shift_b, shift_d, use32, seq, seq_shift, ctypes.addressof(stored), ctypes.addressof(seq_out))
        assert stored.value == own | (seq << seq_shift if seq_shift < (32 if use32 else 64) else 0)
        assert (seq_out.value, back) == (seq, own)


@pytest.mark.parametrize("case", ["zero", "below", "at", "one_over", "mixed", "all_over"])
def test_shard_accounting(fin, case):
    ns = fin.psfm_host_nshard()
    cap = 1000
    cnt = {"zero": [0] * ns, "below": [(7 * k) % cap for k in range(ns)], "at": [cap] * ns,
           "one_over": [cap if k != 5 else cap + 1 for k in range(ns)],
           "mixed": [(0, cap - 1, cap, cap + 1, 3 * cap)[k % 5] for k in range(ns)], "all_over": [cap + 1 + k for k in range(ns)]}[case]
    fin_cnt = (ctypes.c_int * ns)(*cnt)
    count, start, n = (ctypes.c_int * ns)(), (ctypes.c_longlong * ns)(), ctypes.c_longlong(-1)
    over = fin.psfm_host_shard_offsets(ctypes.addressof(fin_cnt), cap, ctypes.addressof(count), ctypes.addressof(start), ctypes.addressof(n))
    kept = [min(c, cap) for c in cnt]
    assert list(count) == kept and n.value == sum(kept)
    assert list(start) == [sum(kept[:k]) for k in range(ns)]
    assert bool(over) == any(c > cap for c in cnt) == (case in ("one_over", "mixed", "all_over"))
