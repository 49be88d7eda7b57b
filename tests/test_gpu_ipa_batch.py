"""GPU: h2_ipa_*_batch_device and ipa.create_proofs -- m openings of the inner product argument in lockstep.

Every opening of a batch has its own polynomial, x3, z, challenges and blinds, so a kernel that reads opening 0's scalars
for opening i gives wrong bytes.  The judges are test_gpu_ipa.py's `reference` (upstream's collapsing algorithm on the C
oracle, byte for byte in every round), the single-opening calls on separate states, and for whole proofs ipa.create_proof,
ipa.verify_proofs and test_gpu_ipa_proof.py's host verifier, which makes no GPU call."""
import ctypes
import random

import numpy as np
import pytest

import test_gpu_ipa as T
import test_gpu_ipa_proof as TP

pytestmark = pytest.mark.gpu

H2_OK, H2_EINVAL, H2_EHANDLE = 0, -1, -4
MAX_K, MAX_BATCH = 20, 64
FF = -1                                               # int64 of 0xFF bytes


def openings(curve, k, count, seed):
    """`count` different openings; the second polynomial is all zero, the third equals the first (with its own scalars)"""
    out = [T.inputs(curve, k, seed + 0x100 * i) for i in range(count)]
    if count > 1:
        out[1]["a"] = [0] * (1 << k)
    if count > 2:
        out[2]["a"] = list(out[0]["a"])
    return out


_REFERENCES = {}


def references(curve, k):
    """five openings of (curve, k) and what upstream's algorithm gives for each: computed once, never changed"""
    key = (curve, k)
    if key not in _REFERENCES:
        ins = openings(curve, k, 5, 0xBA7C + 16 * k)
        _REFERENCES[key] = (ins, [T.reference(curve, k, **I) for I in ins])
    return _REFERENCES[key]


def state_bytes(k, m):
    need = ctypes.c_size_t(0)
    assert T.L().h2_ipa_batch_state_bytes(k, m, ctypes.byref(need)) == H2_OK
    return need.value


class Batch:
    """one caller-owned state buffer, sized for `room` openings, full of 0xFF bytes, never cleared between runs"""

    def __init__(self, curve, k, room):
        import torch
        T.setup(curve, k)
        self.curve, self.k = curve, k
        self.state = torch.full((state_bytes(k, room) // 8,), FF, dtype=torch.int64, device="cuda")
        self.out = torch.zeros((room + 1, 16), dtype=torch.int64, device="cuda")

    def column(self, ins, name, j=None):
        p, _ = T.primes(self.curve)
        return T.mont(p, [I[name] if j is None else I[name][j] for I in ins])

    def begin(self, ins, m=None, k=None, d_p=None, state_ptr=None, cid=None):
        p, _ = T.primes(self.curve)
        self.polys = [T.to_dev(T.mont(p, I["a"])) for I in ins]
        ptrs = (ctypes.c_void_p * max(1, len(ins)))(*([t.data_ptr() for t in self.polys] if d_p is None else d_p))
        if d_p == []:
            ptrs = None                               # no array at all
        x3 = self.column(ins, "x3")
        return T.L().h2_ipa_begin_batch_device(T.CID[self.curve] if cid is None else cid, self.k if k is None else k,
                                               len(ins) if m is None else m, ptrs, x3.ctypes.data,
                                               ctypes.c_void_p(self.state.data_ptr() if state_ptr is None else state_ptr), None)

    def round(self, ins, j, m=None, k=None, handle=None, state_ptr=None, out_ptr=None, drop_u=False, extra_u=False):
        p, _ = T.primes(self.curve)
        S = T.setup(self.curve, self.k)
        jj = min(j, self.k - 1)
        um = ui = None
        if (j and not drop_u) or extra_u:
            um = T.mont(p, [I["us"][max(jj, 1) - 1] for I in ins])
            ui = T.mont(p, [pow(I["us"][max(jj, 1) - 1], -1, p) for I in ins])
        z = self.column(ins, "z")
        lb = T.mont(p, [I["blinds"][jj][0] for I in ins])
        rb = T.mont(p, [I["blinds"][jj][1] for I in ins])
        return T.L().h2_ipa_round_batch_device(T.CID[self.curve], S["bases"].handle if handle is None else handle,
                                               self.k if k is None else k, j, len(ins) if m is None else m,
                                               ctypes.c_void_p(self.state.data_ptr() if state_ptr is None else state_ptr),
                                               um.ctypes.data if um is not None else None, ui.ctypes.data if ui is not None else None,
                                               z.ctypes.data, lb.ctypes.data, rb.ctypes.data,
                                               ctypes.c_void_p(self.out.data_ptr() if out_ptr is None else out_ptr), None)

    def final(self, ins, m=None, k=None, state_ptr=None, out_ptr=None):
        p, _ = T.primes(self.curve)
        um = T.mont(p, [I["us"][-1] for I in ins])
        ui = T.mont(p, [pow(I["us"][-1], -1, p) for I in ins])
        return T.L().h2_ipa_final_batch_device(T.CID[self.curve], self.k if k is None else k, len(ins) if m is None else m,
                                               ctypes.c_void_p(self.state.data_ptr() if state_ptr is None else state_ptr),
                                               um.ctypes.data, ui.ctypes.data,
                                               ctypes.c_void_p(self.out.data_ptr() if out_ptr is None else out_ptr), None)

    def run(self, ins):
        """-> ([per round: (m, 16) limbs L_i || R_i], (m, 8) limbs c_i || b_i[0])"""
        m = len(ins)
        assert self.begin(ins) == H2_OK
        before = [T.from_dev(t).copy() for t in self.polys]
        got = []
        for j in range(self.k):
            assert self.round(ins, j) == H2_OK
            got.append(T.from_dev(self.out)[:m].copy())
        assert self.final(ins) == H2_OK
        cb = T.from_dev(self.out).reshape(-1)[:8 * m].reshape(m, 8).copy()
        for t, b in zip(self.polys, before):
            assert np.array_equal(T.from_dev(t), b), "d_p is only read"
        return got, cb


def check(batch, ins, refs):
    p, _ = T.primes(batch.curve)
    got, cb = batch.run(ins)
    for i, (want_lr, c, b0, _) in enumerate(refs):
        for j in range(batch.k):
            assert np.array_equal(got[j][i, :8], want_lr[j][:8]), "opening %d: L_%d differs" % (i, j)
            assert np.array_equal(got[j][i, 8:], want_lr[j][8:]), "opening %d: R_%d differs" % (i, j)
        assert np.array_equal(cb[i].reshape(2, 4), T.mont(p, [c, b0])), "opening %d: c or b[0] differs" % i


@pytest.mark.parametrize("m", [1, 2, 3, 5])
@pytest.mark.parametrize("k", [1, 2, 4])
@pytest.mark.parametrize("curve", T.CURVES)
def test_the_batch_matches_the_collapsing_algorithm(curve, k, m):
    ins, refs = references(curve, k)
    check(Batch(curve, k, m), ins[:m], refs[:m])


def test_the_largest_batch_matches_the_collapsing_algorithm():
    """m = H2_IPA_MAX_BATCH at k = 2: 128 columns in the round's MSM, every row of the scalar table, blockIdx.y up to 63"""
    curve, k = "pallas", 2
    ins = openings(curve, k, MAX_BATCH, 0x64BA7C)
    check(Batch(curve, k, MAX_BATCH), ins, [T.reference(curve, k, **I) for I in ins])


@pytest.mark.parametrize("curve", ["pallas", "bn254"])
def test_the_batch_matches_three_single_openings(curve):
    """k = 10: half = 512 at j = 0, two partial pairs per opening, and IPA_H_PER's tail in the later rounds"""
    k, m = 10, 3
    ins = openings(curve, k, m, 0x51A6 + T.CID[curve])
    got, cb = Batch(curve, k, m).run(ins)
    for i, I in enumerate(ins):
        lr, one_cb, _ = T.Opening(curve, k).run(**I)
        for j in range(k):
            assert np.array_equal(got[j][i], lr[j]), "opening %d: L_%d || R_%d differs" % (i, j, j)
        assert np.array_equal(cb[i], one_cb), "opening %d: c or b[0] differs" % i


def test_stale_state_of_another_batch_size_changes_nothing():
    curve, k = "vesta", 4
    ins, refs = references(curve, k)
    batch = Batch(curve, k, 5)                        # 0xFF bytes everywhere before the first begin
    check(batch, ins[:5], refs[:5])
    check(batch, ins[3:5], refs[3:5])                 # m = 2 on what m = 5 left: every region lies elsewhere
    check(batch, ins[1:4], refs[1:4])
    batch.state.fill_(FF)
    check(batch, ins[:2], refs[:2])


def test_a_stale_scalar_table_is_not_read_at_m_1():
    """the scalars of a batch of one travel in the kernels' arguments: the table at the end of the m = 1 layout (5 elements)
    holds what m = 2 left there, then 0xFF bytes, and is neither read nor written"""
    curve, k = "vesta", 4
    ins, refs = references(curve, k)
    batch = Batch(curve, k, 5)
    check(batch, ins[:2], refs[:2])
    check(batch, ins[2:3], refs[2:3])                 # m = 1 on what m = 2 left
    end = state_bytes(k, 1) // 8
    batch.state[end - 5 * 4:end] = FF
    check(batch, ins[3:4], refs[3:4])
    assert (batch.state[end - 5 * 4:end] == FF).all().item(), "m = 1 wrote its scalar table"
    check(batch, ins[:2], refs[:2])


@pytest.mark.parametrize("curve,k", [("pallas", 3), ("vesta", 6)])
def test_the_two_spellings_are_one_path(curve, k):
    """one opening on one state, the single calls and the batch calls with m = 1 taking turns: begun by either spelling,
    every round through the other one than the call before, finished by the spelling that began"""
    p, _ = T.primes(curve)
    I = T.inputs(curve, k, 0x2B1 + k)
    want_lr, c, b0, s = T.reference(curve, k, **I)
    batch = Batch(curve, k, 1)
    single = T.Opening(curve, k)
    assert single.state.numel() == batch.state.numel()
    single.state = batch.state                        # ONE state under both spellings
    state = ctypes.c_void_p(batch.state.data_ptr())
    cid = T.CID[curve]
    um = T.mont(p, [I["us"][-1], pow(I["us"][-1], -1, p)])
    for first in ("single", "batch"):
        batch.state.fill_(FF)
        if first == "single":
            d_p = T.to_dev(T.mont(p, I["a"]))
            assert T.L().h2_ipa_begin_device(cid, k, ctypes.c_void_p(d_p.data_ptr()), T.mont(p, [I["x3"]]).ctypes.data, state,
                                             None) == H2_OK
        else:
            assert batch.begin([I]) == H2_OK
        for j in range(k):
            if (j % 2 == 0) == (first == "single"):   # round 0 goes through the spelling that did not begin
                assert batch.round([I], j) == H2_OK
                got = T.from_dev(batch.out)[0]
            else:
                assert single.round(j, I["z"], I["us"], I["blinds"]) == H2_OK
                got = T.from_dev(single.out)
            assert np.array_equal(got[:8], want_lr[j][:8]), "begun by %s: L_%d differs" % (first, j)
            assert np.array_equal(got[8:], want_lr[j][8:]), "begun by %s: R_%d differs" % (first, j)
        if first == "single":
            assert T.L().h2_ipa_final_device(cid, k, state, um[0].ctypes.data, um[1].ctypes.data,
                                             ctypes.c_void_p(single.out.data_ptr()), ctypes.c_void_p(single.s_out.data_ptr()),
                                             None) == H2_OK
            cb = T.from_dev(single.out)[:8]
            assert np.array_equal(T.from_dev(single.s_out), T.mont(p, s)), "the finished s differs"
        else:
            assert batch.final([I]) == H2_OK
            cb = T.from_dev(batch.out).reshape(-1)[:8]
        assert np.array_equal(cb.reshape(2, 4), T.mont(p, [c, b0])), "begun by %s: c or b[0] differs" % first


def test_argument_errors_then_a_valid_batch():
    import halo2_prover_amd as h2
    curve, k, m = "pallas", 4, 3
    ins, refs = references(curve, k)
    ins, refs = ins[:m], refs[:m]
    S = T.setup(curve, k)
    batch = Batch(curve, k, MAX_BATCH)               # room for the largest batch: a refused larger one could not be blamed on it
    check(batch, ins, refs)
    short = h2.Bases(curve, np.concatenate([S["g"]]))                    # 2^k bases instead of 2^k + 2
    other = T.setup("vesta", k)["bases"]                                 # the right size, another curve
    good = [t.data_ptr() for t in batch.polys]
    state, out = batch.state.data_ptr(), batch.out.data_ptr()
    too_many = [ins[i % m] for i in range(MAX_BATCH + 1)]
    refused = [
        ("begin m = 0", lambda: batch.begin(ins, m=0), H2_EINVAL),
        ("begin m > max", lambda: batch.begin(too_many), H2_EINVAL),
        ("begin k = 0", lambda: batch.begin(ins, k=0), H2_EINVAL),
        ("begin k > max", lambda: batch.begin(ins, k=MAX_K + 1), H2_EINVAL),
        ("begin unknown curve", lambda: batch.begin(ins, cid=7), H2_EINVAL),
        ("begin null state", lambda: batch.begin(ins, state_ptr=0), H2_EINVAL),
        ("begin misaligned state", lambda: batch.begin(ins, state_ptr=state + 8), H2_EINVAL),
        ("begin null d_p", lambda: batch.begin(ins, d_p=[]), H2_EINVAL),
        ("begin null d_p[1]", lambda: batch.begin(ins, d_p=[good[0], None, good[2]]), H2_EINVAL),
        ("begin misaligned d_p[2]", lambda: batch.begin(ins, d_p=[good[0], good[1], good[2] + 8]), H2_EINVAL),
        ("round m = 0", lambda: batch.round(ins, 0, m=0), H2_EINVAL),
        ("round m > max", lambda: batch.round(too_many, 0), H2_EINVAL),
        ("round k = 0", lambda: batch.round(ins, 0, k=0), H2_EINVAL),
        ("round k > max", lambda: batch.round(ins, 0, k=MAX_K + 1), H2_EINVAL),
        ("round j = k", lambda: batch.round(ins, k), H2_EINVAL),
        ("round null state", lambda: batch.round(ins, 0, state_ptr=0), H2_EINVAL),
        ("round misaligned state", lambda: batch.round(ins, 0, state_ptr=state + 8), H2_EINVAL),
        ("round null out", lambda: batch.round(ins, 0, out_ptr=0), H2_EINVAL),
        ("round misaligned out", lambda: batch.round(ins, 0, out_ptr=out + 8), H2_EINVAL),
        ("round u_prev missing at j = 1", lambda: batch.round(ins, 1, drop_u=True), H2_EINVAL),
        ("round u_prev superfluous at j = 0", lambda: batch.round(ins, 0, extra_u=True), H2_EINVAL),
        ("round table of 2^k bases", lambda: batch.round(ins, 0, handle=short.handle), H2_EINVAL),
        ("round table of another curve", lambda: batch.round(ins, 0, handle=other.handle), H2_EINVAL),
        ("round table of another k", lambda: batch.round(ins, 0, handle=T.setup(curve, 2)["bases"].handle), H2_EINVAL),
        ("round unregistered handle", lambda: batch.round(ins, 0, handle=0x7FFFFFFF12345), H2_EHANDLE),
        ("final m = 0", lambda: batch.final(ins, m=0), H2_EINVAL),
        ("final m > max", lambda: batch.final(too_many), H2_EINVAL),
        ("final k = 0", lambda: batch.final(ins, k=0), H2_EINVAL),
        ("final k > max", lambda: batch.final(ins, k=MAX_K + 1), H2_EINVAL),
        ("final null state", lambda: batch.final(ins, state_ptr=0), H2_EINVAL),
        ("final misaligned state", lambda: batch.final(ins, state_ptr=state + 8), H2_EINVAL),
        ("final null out", lambda: batch.final(ins, out_ptr=0), H2_EINVAL),
        ("final misaligned out", lambda: batch.final(ins, out_ptr=out + 8), H2_EINVAL),
    ]
    for what, call, want in refused:
        assert call() == want, what
        check(batch, ins, refs)                       # nothing was enqueued: the next valid batch gives the right bytes
    short.release()
    assert batch.round(ins, 0, handle=short.handle) == H2_EHANDLE      # released: not registered any more
    check(batch, ins, refs)


# ---- whole proofs ----------------------------------------------------------------------------------------------------
_ITEMS = {}


def proof_items(curve, k, m):
    """m polynomials on test_gpu_ipa_proof.py's params of (curve, k), each with its blind, point, value and commitment"""
    key = (curve, k, m)
    if key not in _ITEMS:
        C = TP.case(curve, k)
        params, p, n = C["params"], C["params"].p, 1 << k
        R = (1 << 256) % p
        rnd = random.Random(0xBA7C4 + k + m)
        out = []
        for _ in range(m):
            poly = [rnd.randrange(p) for _ in range(n)]
            s_poly = [rnd.randrange(p) for _ in range(n)]
            x3 = rnd.randrange(1, p)
            D = dict(C)
            D.update(poly_m=TP.limbs([c * R % p for c in poly]), s_m=TP.limbs([c * R % p for c in s_poly]), blind=rnd.randrange(p),
                     x3=x3, v=sum(c * pow(x3, i, p) for i, c in enumerate(poly)) % p)
            D["P"] = params.commit(D["poly_m"], D["blind"])
            out.append(D)
        _ITEMS[key] = out
    return _ITEMS[key]


@pytest.mark.parametrize("with_s_poly", [True, False])
@pytest.mark.parametrize("curve,k,m", [("pallas", 4, 3), ("vesta", 4, 3), ("pallas", 10, 2)])
def test_create_proofs_gives_create_proofs_bytes(curve, k, m, with_s_poly):
    import halo2_prover_amd as h2
    from halo2_prover_amd import ipa
    Cs = proof_items(curve, k, m)
    params = Cs[0]["params"]

    def item(i, C):
        return (h2.Blake2bTranscript(curve), C["poly_m"], C["blind"], C["x3"], TP.Rng(0x5EED + i), C["s_m"] if with_s_poly else None)

    trs = [item(i, C) for i, C in enumerate(Cs)]
    proofs = ipa.create_proofs(params, trs)
    assert len(proofs) == m and len(set(proofs)) == m
    for i, C in enumerate(Cs):
        single = item(i, C)
        assert proofs[i] == ipa.create_proof(params, *single), "proof %d is not create_proof's" % i
        assert bytes(trs[i][0].bytes) == bytes(single[0].bytes), "transcript %d is not left where create_proof leaves it" % i
    readers = [(h2.Blake2bTranscript(curve, proofs[i]), C["P"], C["x3"], C["v"]) for i, C in enumerate(Cs)]
    assert ipa.verify_proofs(params, readers) == [True] * m
    for i, C in enumerate(Cs):
        assert TP.host_verify(C, proofs[i], C["v"]), "the host verifier refuses proof %d" % i
    assert not TP.host_verify(Cs[-1], TP.flip(proofs[-1], 32 * (1 + 2 * k)), Cs[-1]["v"])      # one bit of c
    assert not TP.host_verify(Cs[0], proofs[1], Cs[0]["v"])                                    # another opening's proof


def test_create_proofs_beyond_the_largest_batch():
    """65 items at k = 4: a full group of H2_IPA_MAX_BATCH and a group of one; host arrays of 64 x 32 bytes and more, which
    the allocator does not keep intact once they are freed; s_poly given for the even items, drawn for the odd ones"""
    import halo2_prover_amd as h2
    from halo2_prover_amd import ipa
    curve, k, m = "pallas", 4, MAX_BATCH + 1
    Cs = proof_items(curve, k, m)
    params = Cs[0]["params"]

    def item(i, C):
        return (h2.Blake2bTranscript(curve), C["poly_m"], C["blind"], C["x3"], TP.Rng(0x65ED + i), C["s_m"] if i % 2 == 0 else None)

    proofs = ipa.create_proofs(params, [item(i, C) for i, C in enumerate(Cs)])
    assert len(proofs) == m
    for i, C in enumerate(Cs):
        assert proofs[i] == ipa.create_proof(params, *item(i, C)), "proof %d is not create_proof's" % i
    readers = [(h2.Blake2bTranscript(curve, proofs[i]), C["P"], C["x3"], C["v"]) for i, C in enumerate(Cs)]
    assert ipa.verify_proofs(params, readers) == [True] * m
    for i in (0, MAX_BATCH - 1, MAX_BATCH):
        assert TP.host_verify(Cs[i], proofs[i], Cs[i]["v"]), "the host verifier refuses proof %d" % i


def test_create_proofs_of_nothing():
    from halo2_prover_amd import ipa
    assert ipa.create_proofs(TP.case("pallas", 4)["params"], []) == []
