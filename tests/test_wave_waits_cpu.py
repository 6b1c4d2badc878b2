"""What a wave of the fused narrow kernels (gnx_wave_kernel.h: block_wave_body) waits for between its edge phase and its node phase, read from the
compiler's assembly of gnx_narrow.hip for gfx950 (compiled once per session, as build.py compiles it):

  * no wait for the ef' stores: between the wave barrier that ends the edge phase and the nf' store there is no s_waitcnt whose vmcnt is lower
    than the number of ef' stores the edge phase can have outstanding (vmcnt counts stores on this target; a full vmcnt(0) in front of the
    segmented sum made every wave sit out the acknowledgement of its own stores);
  * the segmented edge->node sum reads a batch of rows from LDS per s_waitcnt lgkmcnt: four where the kernel has the registers
    (gnx_wave_kernel.h: seg_batch), in one round trip.

Every ahead-of-time fp32 kernel built from the body: k_block_wave (plain, CHAIN, PACK, LayerNorm on load; one graph or several; 1, 2 and 4 edges
per lane), k_block_wave_run and k_block_wave_carry.  The FFE form stores its edge rows at the end of the kernel and keeps the one-row loop.

Left waiting, by name: k_block_wave<..., LN = true> (the block of a narrow GNCore when its edge FeedForward is not fused: LayerNorm on load).
The fix is a wait for every load in front of the edge products; with LayerNorm on load the first rows are normalised while the gathered
rows are still on their way, and the wait would end that overlap in a kernel bound by instruction issue.  Its segmented sum is batched like
the others'."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "graphnets.jl_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

NAME = re.compile(r"^_ZN3gnx\d+(k_block_wave(?:_run|_carry)?)I((?:Li\d+E){6})((?:Lb[01]E)+)EEv")


def seg_batch(de, dn, oe, ept):
    """gnx_wave_kernel.h: seg_batch for the fp32, non-FFE forms — the sets that stay below four rows per trip, and why.
    One row per trip: fewer than a dozen values per lane in the edge phase ((0,2,0)=>(2,2), (2,2,2)=>(2,2), and one edge per lane at (3,4,5) and
    (4,3,2)) — a batch of two cost a register or scratch; ef' wider than 4 ((10,5,x)=>(10,5), (8,8,8)=>(16,8)) — four rows cost up to 21
    registers, and those kernels are bound by vector issue.  Two rows: one edge per lane otherwise (four cost registers, two do not)."""
    if oe > 4 or ept * (de + dn) < 12:
        return 1
    if ept == 1:
        return 2
    return 4


@pytest.fixture(scope="session")
def kernels(tmp_path_factory):
    """kernel name -> its assembly lines, of every kernel built from block_wave_body in gnx_narrow.hip"""
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    out = tmp_path_factory.mktemp("wave_waits") / "gnx_narrow.s"
    cmd = [HIPCC, "-x", "hip", "-S", "--cuda-device-only", "-O3", "--offload-arch=gfx950", "-std=c++17", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC,
           "-fno-gpu-rdc", "-o", str(out), os.path.join(CSRC, "gnx_narrow.hip")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=1200)
    assert r.returncode == 0, r.stderr[-3000:]
    return _split(open(out))


def _split(lines):
    found, name, body = {}, None, []
    for ln in lines:
        if name is None:
            m = re.match(r"^(_ZN3gnx\S+):", ln)
            if m and NAME.match(m.group(1)):
                name, body = m.group(1), []
        elif ln.startswith(".Lfunc_end"):
            found[name] = body
            name = None
        else:
            body.append(ln.rstrip("\n"))
    return found


def _params(name):
    m = NAME.match(name)
    ints = [int(v) for v in re.findall(r"Li(\d+)E", m.group(2))]
    bools = [v == "1" for v in re.findall(r"Lb([01])E", m.group(3))]
    kind = m.group(1)
    ffe = kind == "k_block_wave" and bools[3]
    return kind, ints, bools, ffe


def _phases(body):
    """(edge phase, node phase up to and including the nf' store): the lines between the body's two wave barriers — the first pair of neighbouring
    wave barriers with global stores between them (the graph updates of the CHAIN and PACK forms have wave barriers of their own, behind the
    tile program) — and from the second one to the first global store behind it"""
    bars = [i for i, ln in enumerate(body) if ln.strip() == "; wave barrier"]
    pairs = [(a, b) for a, b in zip(bars, bars[1:]) if any("global_store" in ln for ln in body[a:b])]
    assert pairs, f"{len(bars)} wave barriers, none with stores between them"
    a, b = pairs[0]
    store = next(i for i in range(b, len(body)) if "global_store" in body[i])
    return body[a:b], body[b:store + 1]


def _vmcnt(ln):
    m = re.search(r"s_waitcnt.*vmcnt\((\d+)\)", ln)
    return int(m.group(1)) if m else None


DWORDS = {"ds_read_b32": 1, "ds_read2_b32": 2, "ds_read_b64": 2, "ds_read2_b64": 4, "ds_read_b96": 3, "ds_read_b128": 4}


def _lds_loops(lines):
    """the innermost loops of `lines` that read LDS: (dwords read per trip, LDS round trips per trip) per loop — a round trip is a run of reads
    closed by an s_waitcnt lgkmcnt (counted waits behind the last read of a run drain ONE batch: they are no further trips)"""
    labels = {ln.split(":")[0]: i for i, ln in enumerate(lines) if re.match(r"^\.LBB\d+_\d+:", ln)}
    loops = []
    for i, ln in enumerate(lines):
        m = re.match(r"\s+s_cbranch_\w+\s+(\.LBB\d+_\d+)", ln)
        if m and m.group(1) in labels and labels[m.group(1)] < i:
            loops.append((labels[m.group(1)], i))
    inner = [l for l in loops if not any(o != l and l[0] <= o[0] and o[1] <= l[1] for o in loops)]
    out = []
    for a, b in inner:
        seg = lines[a:b]
        d = sum(DWORDS[t.split()[0]] for t in seg if t.split() and t.split()[0] in DWORDS)
        for t in seg:
            assert not (t.split() and t.split()[0].startswith("ds_read") and t.split()[0] not in DWORDS), t
        if d:
            trips, reading = 0, False
            for t in seg:
                if t.split() and t.split()[0] in DWORDS:
                    reading = True
                elif reading and "s_waitcnt" in t and "lgkmcnt" in t:
                    trips, reading = trips + 1, False
            out.append((d, trips))
    return out


def test_every_form_is_there(kernels):
    kinds = {}
    for n in kernels:
        kind, ints, bools, ffe = _params(n)
        kinds.setdefault(kind, []).append((ints, bools))
    assert set(kinds) == {"k_block_wave", "k_block_wave_run", "k_block_wave_carry"}, sorted(kinds)
    plain = kinds["k_block_wave"]  # bools: LN, ONEG, PACK, FFE, CHAIN, BF16
    for what, sel in (("CHAIN", lambda b: b[4]), ("PACK", lambda b: b[2]), ("ONEG", lambda b: b[1]), ("several graphs", lambda b: not b[1]), ("LN", lambda b: b[0])):
        assert any(sel(b) for _, b in plain), what
    assert {i[5] for i, _ in plain} >= {1, 2}
    assert all(not b[5] for _, b in plain), "a bf16 kernel in the fp32 file"
    assert any(i[:5] == [10, 5, 0, 3, 4] and b[0] for i, b in kinds["k_block_wave_run"]) and any(i[:5] == [10, 5, 0, 3, 4] for i, _ in kinds["k_block_wave_carry"])


def test_no_wait_for_the_edge_stores_before_the_node_store(kernels):
    bad, seen = [], 0
    for n, body in sorted(kernels.items()):
        kind, ints, bools, ffe = _params(n)
        if ffe or (kind == "k_block_wave" and bools[0]):
            continue  # LEFT WAITING, see the module's text: the LayerNorm-on-load forms (LN = 1, here (10,5,3) => (10,5,x), one graph and several)
        edge, node = _phases(body)
        stores = sum(1 for ln in edge if "global_store" in ln)  # (every copy of the chunk program the compiler made: at least what one path issues)
        assert stores >= 1, n
        seen += 1
        for ln in node:
            v = _vmcnt(ln)
            if v is not None and v < stores:
                bad.append(f"{n}: '{ln.strip()}' with up to {stores} ef' stores outstanding")
    assert seen >= 100, seen
    assert not bad, "\n".join(bad)


def test_segmented_sum_reads_a_batch_of_rows_per_wait(kernels):
    bad, seen4 = [], 0
    for n, body in sorted(kernels.items()):
        kind, ints, bools, ffe = _params(n)
        de, dn, dg, oe, on, ept = ints
        if ffe or oe == 0:
            continue
        _, node = _phases(body)
        loops = _lds_loops(node)
        want = seg_batch(de, dn, oe, ept)
        seen4 += want == 4
        if len(loops) != 1:
            bad.append(f"{n}: {len(loops)} LDS loops in the node phase")
            continue
        dwords, trips = loops[0]
        if trips != 1 or dwords != want * oe:
            bad.append(f"{n}: {dwords} dwords ({dwords / oe:g} rows of {oe}) in {trips} LDS round trips per trip of the loop, expected {want} rows in one")
    assert seen4 >= 20, seen4
    assert not bad, "\n".join(bad)
