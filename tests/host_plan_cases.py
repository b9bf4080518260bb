"""How the host-pointer entry points of the C ABI (pem_cathode_f64, pem_thruster_f64, pem_plume_f64, pem_coupled_f64) cut a
call into chunks and move a chunk's data, restated in plain Python from the rules include/pem_hip.h documents, and the table
of sizes at which tests/test_host_entry_points_host.py (no GPU) and tests/test_host_entry_points.py (GPU) hold them.

The rules: a call is cut into chunks; one chunk's arrays are carved from a workspace, each padded to 256 bytes, the inputs
first (they end at `in_end`), the outputs after them (they end at `footprint`).  `reserve` is what the call asks the
workspace for: the footprint, except for the thruster stage, which always asks for room for all eight outputs.
    regime 0  reserve <= ZC_BYTES and PEM_ZERO_COPY is not 0: the kernels work on the pinned buffer
    regime 1  footprint <= STAGE_BYTES: one copy each way through the pinned mirror
    regime 2  in_end <= STAGE_BYTES < footprint: the inputs in one copy, the outputs array by array
    regime 3  one copy per array
"""
import ctypes as C
from collections import namedtuple

import numpy as np

CATHODE, THRUSTER, PLUME, COUPLED = 0, 1, 2, 3          # PEM_HOST_* of include/pem_hip.h
NAMES = {CATHODE: 'cathode', THRUSTER: 'thruster', PLUME: 'plume', COUPLED: 'coupled'}
ZC_BYTES = 256 << 10
STAGE_BYTES = 2 << 20
NANG = 91

Plan = namedtuple('Plan', 'chunk n_chunks in_end footprint reserve regime')


def padded(nbytes):
    return (nbytes + 255) // 256 * 256


def chunk_size(entry, n, R=1):
    """the three chunk rules"""
    if entry in (CATHODE, THRUSTER):
        return min(n, 1 << 24)
    if entry == PLUME:
        c = min(max(1024, (1 << 28) // (NANG * R * 8)), n)
    else:
        c = min((1 << 28) // (NANG * 8), n)
    return (c + 63) // 64 * 64


def array_bytes(entry, chunk, R=1, n_optional=8):
    """(bytes of every input array, bytes of every output array) of one chunk, in carving order"""
    d = 8 * chunk
    if entry == CATHODE:
        return [d] * 6, [d]
    if entry == THRUSTER:
        return [d] * 4, [d] * n_optional
    if entry == PLUME:                                   # T among the inputs, T_c and invalid among the outputs: always carved
        return [d] * 10, [d * NANG * R, d * R, d * R, chunk]
    return [d] * 15, [d] * 5 + [chunk, d * NANG]          # V_cc I_B0 T div_angle T_c, invalid, j_ion


def plan(entry, n, R=1, n_optional=8, zero_copy=True):
    chunk = chunk_size(entry, n, R)
    ins, outs = array_bytes(entry, chunk, R, n_optional)
    in_end = sum(padded(b) for b in ins)
    footprint = in_end + sum(padded(b) for b in outs)
    reserve = in_end + 8 * padded(8 * chunk) if entry == THRUSTER else footprint
    if zero_copy and reserve <= ZC_BYTES:
        regime = 0
    elif footprint <= STAGE_BYTES:
        regime = 1
    elif in_end <= STAGE_BYTES:
        regime = 2
    else:
        regime = 3
    return Plan(chunk, -(-n // chunk), in_end, footprint, reserve, regime)


Boundary = namedtuple('Boundary', 'entry R n_optional low regime_low regime_high')     # high side: low + 1

# Every regime boundary a call can reach, worked out by hand from the rules above: `low` is the largest n that still takes
# regime_low, low + 1 takes regime_high.  A regime that no n reaches leaves no row:
#   thruster without outputs: footprint == in_end, so it goes from 1 straight to 3
#   plume, R = 8: 64 samples (the smallest chunk) already exceed ZC_BYTES
#   plume, R = 25: the same, and the chunk stops growing at 14 784 samples, before the inputs reach STAGE_BYTES
#   cathode: 7 padded(8 n) <= 256 KiB <=> padded(8 n) <= 146 * 256 <=> n <= 4672;  <= 2 MiB <=> n <= 37 440;
#            6 padded(8 n) <= 2 MiB <=> padded(8 n) <= 1365 * 256 <=> n <= 43 680
#   thruster: 12 padded(8 n) <= 256 KiB <=> n <= 2720 whatever the outputs; (4 + k) padded(8 n) <= 2 MiB <=> n <= 21 824 (k = 8),
#            52 416 (k = 1), 65 536 (k = 0); 4 padded(8 n) <= 2 MiB <=> n <= 65 536
#   coupled (chunks of 64 c): 20 * 512 c + 46 592 c + padded(64 c) <= 256 KiB <=> c <= 4; <= 2 MiB <=> c <= 36;
#            15 * 512 c <= 2 MiB <=> c <= 273
#   plume (chunks of 64 c: 10 * 512 c of inputs, then 46 592 R c + 2 padded(512 R c) + padded(64 c)):
#            R = 1: 52 736 c + padded(64 c) <= 256 KiB <=> c <= 4; <= 2 MiB <=> c <= 39;  R = 3: 145 920 c + ... <=> c <= 1, c <= 14;
#            R = 8: 386 048 c + ... <= 2 MiB <=> c <= 5;  R = 25: 1 195 520 c + ... <=> c <= 1;  5120 c <= 2 MiB <=> c <= 409
BOUNDARIES = [
    Boundary(PLUME, 1, 0, 256, 0, 1), Boundary(PLUME, 1, 0, 2496, 1, 2), Boundary(PLUME, 1, 0, 26176, 2, 3),
    Boundary(PLUME, 3, 0, 64, 0, 1), Boundary(PLUME, 3, 0, 896, 1, 2), Boundary(PLUME, 3, 0, 26176, 2, 3),
    Boundary(PLUME, 8, 0, 320, 1, 2), Boundary(PLUME, 8, 0, 26176, 2, 3),
    Boundary(PLUME, 25, 0, 64, 1, 2),
    Boundary(CATHODE, 1, 0, 4672, 0, 1), Boundary(CATHODE, 1, 0, 37440, 1, 2), Boundary(CATHODE, 1, 0, 43680, 2, 3),
    Boundary(THRUSTER, 1, 8, 2720, 0, 1), Boundary(THRUSTER, 1, 8, 21824, 1, 2), Boundary(THRUSTER, 1, 8, 65536, 2, 3),
    Boundary(THRUSTER, 1, 1, 2720, 0, 1), Boundary(THRUSTER, 1, 1, 52416, 1, 2), Boundary(THRUSTER, 1, 1, 65536, 2, 3),
    Boundary(THRUSTER, 1, 0, 2720, 0, 1), Boundary(THRUSTER, 1, 0, 65536, 1, 3),
    Boundary(COUPLED, 1, 0, 256, 0, 1), Boundary(COUPLED, 1, 0, 2304, 1, 2), Boundary(COUPLED, 1, 0, 17472, 2, 3),
]

# one chunk / two chunks: `chunk` samples fill the first chunk, chunk + 1 leave one sample for the second
TwoChunks = namedtuple('TwoChunks', 'entry R chunk regime')
TWO_CHUNKS = [
    TwoChunks(COUPLED, 1, 368768, 3),            # 2^28 // 728 = 368 730, rounded up to 64
    TwoChunks(PLUME, 8, 46144, 3),               # 2^28 // 5824 = 46 091
    TwoChunks(PLUME, 300, 1280, 2),              # 2^28 // 218 400 = 1229: above the floor of 1024; R > 256 takes the generic kernel
    TwoChunks(PLUME, 3000, 1024, 2),             # 2^28 // 2 184 000 = 122: the floor of 1024 (plan only: 2 GB of profile)
    TwoChunks(CATHODE, 1, 1 << 24, 3),           # plan only: more than 900 MB of workspace
    TwoChunks(THRUSTER, 1, 1 << 24, 3),          # plan only
]


def boundaries(entry, R=1, n_optional=0):
    return [b for b in BOUNDARIES if (b.entry, b.R) == (entry, R) and (entry != THRUSTER or b.n_optional == n_optional)]


def find_boundaries(entry, R=1, n_optional=8):
    """(low, regime_low, regime_high) of every regime change of the restated plan within the first chunk, by bisection: the
    chunk, and with it every carved array, grows with n, so the regime never goes back"""
    found, lo = [], 1
    top = chunk_size(entry, 1 << 40, R)
    nopt = n_optional if entry == THRUSTER else 8
    while plan(entry, lo, R, nopt).regime != plan(entry, top, R, nopt).regime:
        a, b, r = lo, top, plan(entry, lo, R, nopt).regime
        while b - a > 1:
            m = (a + b) // 2
            a, b = (m, b) if plan(entry, m, R, nopt).regime == r else (a, m)
        found.append((a, r, plan(entry, b, R, nopt).regime))
        lo = b
    return found


# ---- calling the four entry points through ctypes, with guarded outputs ------------------------------------------------------------
INPUTS = {
    CATHODE: ('P_b', 'V_a', 'T_e', 'V_vac', 'Pstar', 'P_T'),
    THRUSTER: ('V_a', 'V_cc', 'mdot_a', 'a_1'),
    PLUME: ('P_b', 'c0', 'c1', 'c2', 'c3', 'c4', 'c5', 'sigma_cex', 'I_B0', 'T'),          # T is optional
    COUPLED: ('P_b', 'V_a', 'T_e', 'V_vac', 'Pstar', 'P_T', 'mdot_a', 'a_1', 'c0', 'c1', 'c2', 'c3', 'c4', 'c5', 'sigma_cex'),
}
OUTPUTS = {                                                                                 # in the order of the C arguments
    CATHODE: ('V_cc',),
    THRUSTER: ('I_B0', 'I_d', 'T', 'eta_c', 'eta_m', 'eta_v', 'eta_a', 'v_exh'),
    PLUME: ('j_ion', 'div_angle', 'T_c', 'invalid'),
    COUPLED: ('V_cc', 'I_B0', 'T', 'j_ion', 'div_angle', 'T_c', 'invalid'),
}
OPTIONAL = {CATHODE: (), THRUSTER: OUTPUTS[THRUSTER], PLUME: ('T_c', 'invalid'), COUPLED: ('I_B0', 'T', 'j_ion', 'invalid')}
HOST_FN = {CATHODE: 'pem_cathode_f64', THRUSTER: 'pem_thruster_f64', PLUME: 'pem_plume_f64', COUPLED: 'pem_coupled_f64'}
TORR_2_PA = 133.322             # a run-time argument of every entry point: the same on both sides
RADIUS = 1.0                     # the coupled model's sweep radius
GUARD = 17                       # rows every host output is longer than it needs to be
SENTINEL_F64 = 0x7FFCDEADBEEF0011   # a NaN no kernel produces
SENTINEL_U8 = 0xA5


def radii_of(R):
    return np.linspace(0.4, 2.0, R) if R > 1 else np.array([1.0])


def row_len(entry, name, R=1):
    """doubles (bytes for `invalid`) per sample of an output"""
    if name == 'j_ion':
        return NANG * R
    return R if entry == PLUME and name in ('div_angle', 'T_c') else 1


def alloc_outputs(entry, n, R=1, wanted=None):
    """the wanted outputs (default: all), each GUARD rows too long and filled with the sentinel"""
    outs = {}
    for name in OUTPUTS[entry]:
        if wanted is not None and name not in wanted:
            continue
        count = (n + GUARD) * row_len(entry, name, R)
        if name == 'invalid':
            outs[name] = np.full(count, SENTINEL_U8, dtype=np.uint8)
        else:
            outs[name] = np.full(count, SENTINEL_F64, dtype=np.uint64).view(np.float64)
    return outs


def untouched(a):
    """every element still the sentinel"""
    return bool(np.all(a == SENTINEL_U8)) if a.dtype == np.uint8 else bool(np.all(a.view(np.uint64) == SENTINEL_F64))


def _ptr(a):
    return None if a is None else C.c_void_p(a.ctypes.data)


def host_args(entry, n, x, outs, R=1):
    """the argument list of the host-pointer entry point: x and outs map names to arrays, a missing name is passed as NULL"""
    i = [_ptr(x.get(k)) for k in INPUTS[entry]]
    o = [_ptr(outs.get(k)) for k in OUTPUTS[entry]]
    if entry == CATHODE:
        return [n] + i + [TORR_2_PA] + o
    if entry == THRUSTER:
        return [n] + i + o
    if entry == PLUME:
        return [n, R, _ptr(x.get('radii', radii_of(R))), TORR_2_PA] + i + o
    return [n, TORR_2_PA, RADIUS] + i + o


def call_host(lib, entry, n, x, outs, R=1):
    x = dict(x)
    x.setdefault('radii', radii_of(R))                    # kept alive until the call returns
    return getattr(lib, HOST_FN[entry])(*host_args(entry, n, x, outs, R))


def plain_inputs(entry, n):
    return {k: np.full(n, 1.0) for k in INPUTS[entry]}


def malformed_calls(n=5):
    """(label, entry, R, x, names of the outputs passed) of every call the entry points refuse before they look for a device"""
    cases = []
    for entry in (CATHODE, THRUSTER, PLUME, COUPLED):
        required_out = [k for k in OUTPUTS[entry] if k not in OPTIONAL[entry]]
        for k in INPUTS[entry]:
            if entry == PLUME and k == 'T':
                continue
            x = plain_inputs(entry, n)
            del x[k]
            cases.append((f'{NAMES[entry]}: {k} NULL', entry, 1, x, OUTPUTS[entry]))
        for k in required_out:
            cases.append((f'{NAMES[entry]}: {k} NULL', entry, 1, plain_inputs(entry, n), [o for o in OUTPUTS[entry] if o != k]))
    x = plain_inputs(PLUME, n)
    cases.append(('plume: T_c without T', PLUME, 1, {k: v for k, v in x.items() if k != 'T'}, OUTPUTS[PLUME]))
    cases.append(('plume: T without T_c', PLUME, 1, x, ('j_ion', 'div_angle', 'invalid')))
    cases.append(('plume: no radius', PLUME, 0, x, OUTPUTS[PLUME]))
    x = dict(x)
    x['radii'] = None
    cases.append(('plume: radii NULL', PLUME, 1, x, OUTPUTS[PLUME]))
    return cases
