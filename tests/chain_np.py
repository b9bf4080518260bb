"""numpy / long-double restatements of the component chain of pem_sparse_predict_chain_f64_dev (csrc/pem_surrogate.hip).  TEST
INFRASTRUCTURE: each stage is oracle/surrogate_np.predict (or tests/hp_reference.predict_ref), the coupling maps are
t = 2 (y - lo) / w - 1 into the stage's slot of the shared coordinate table."""
import numpy as np


def coupling_coord(y, lo, w):
    return 2.0 * (y - lo) / w - 1.0


def compose(stages, t_ext, vcc_slot, ib0_slot, vcc_map, ib0_map):
    """stages: three (index_set, coefs, values) of oracle/surrogate_np.predict, betas over the n_dim shared slots; t_ext: [n_ext][n]
    coordinates of the other slots in order -> rows V_cc, I_B0, T, div_angle, T_c, plume outputs 1..  (float64)"""
    from oracle import surrogate_np as snp
    n_dim = t_ext.shape[0] + 2
    t = np.zeros((n_dim, t_ext.shape[1]))
    t[[d for d in range(n_dim) if d not in (vcc_slot, ib0_slot)]] = t_ext
    vcc = snp.predict(*stages[0], t)[0]
    t[vcc_slot] = coupling_coord(vcc, *vcc_map)
    thr = snp.predict(*stages[1], t)
    t[ib0_slot] = coupling_coord(thr[0], *ib0_map)
    plu = snp.predict(*stages[2], t)
    return np.concatenate([np.stack([vcc, thr[0], thr[1], plu[0], thr[1] * np.cos(plu[0])]), plu[1:]])


def compose_ld(stages, t_ext, vcc_slot, ib0_slot, vcc_map, ib0_map):
    """the same in np.longdouble through tests/hp_reference.predict_ref; stages: three (betas, coefs, values-per-beta) lists"""
    import hp_reference as hp
    LD = hp.LD
    n_dim = t_ext.shape[0] + 2
    t = np.zeros((n_dim, t_ext.shape[1]), dtype=LD)
    t[[d for d in range(n_dim) if d not in (vcc_slot, ib0_slot)]] = np.asarray(t_ext, dtype=np.float64).astype(LD)
    vcc = hp.predict_ref(*stages[0], t)[0][0]
    t[vcc_slot] = coupling_coord(vcc, LD(vcc_map[0]), LD(vcc_map[1]))
    thr = hp.predict_ref(*stages[1], t)[0]
    t[ib0_slot] = coupling_coord(thr[0], LD(ib0_map[0]), LD(ib0_map[1]))
    plu = hp.predict_ref(*stages[2], t)[0]
    return np.concatenate([np.stack([vcc, thr[0], thr[1], plu[0], thr[1] * np.cos(plu[0])]), plu[1:]])
