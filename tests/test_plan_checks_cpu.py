"""The plan (coeff_off, n_spl, degree, knots, n_knots, inv_T) is held to ONE rule by every glue entry of include/omgx.h that takes it
(the comment above omgx_store_spec), and the part of the rule that needs no handle is judged ahead of the "null handle" answer: every
entry is called here with a null handle and dummy pointers that are never dereferenced -- no device."""
import ctypes as C

import numpy as np

INVALID = -1                                               # OMGX_E_INVALID
PLAN = dict(coeff_off=0, n_spl=2, degree=3, n_knots=18, inv_T=0.1, knots=True)


def _entries():
    """name -> (who, min_degree, has n_spl, n_spl <= 64, has inv_T, call(plan) -> return code)"""
    import omgtools.backend as be
    lib = be.load_library()
    mem = np.zeros(64)
    d, knots = mem.ctypes.data, np.r_[np.zeros(3), np.linspace(0., 1., 12), np.ones(26)]      # (41 doubles: n_knots = 41 stays inside)
    dev = be.PTR_DEVICE | be.BOUNDS_DEVICE

    def kn(pl):
        return knots.ctypes.data if pl['knots'] else None

    def store(pl):
        return C.byref(be.CStoreSpec(out=d, v_tot=None, t0=d, knots=kn(pl), coeff_off=pl['coeff_off'], n_spl=pl['n_spl'], degree=pl['degree'],
                                     n_knots=pl['n_knots'], n_der=1, n_samp=5, dt=0.01, inv_T=pl['inv_T']))

    def signals(pl):
        return C.byref(be.CSignalsSpec(log=d, count=d, overflow=None, knots=kn(pl), coeff_off=pl['coeff_off'], n_spl=pl['n_spl'], degree=pl['degree'],
                                       n_knots=pl['n_knots'], n_der=1, n_samp=10, cap=121, p_t=0, sample_time=0.01, inv_T=pl['inv_T']))

    def plant(pl):
        return C.byref(be.CPlantSpec(state=d, state_prev=d, input_last=d, dist=None, n_upd=d, overflow=None, under_way=None, knots=kn(pl),
                                     coeff_off=pl['coeff_off'], n_spl=pl['n_spl'], degree=pl['degree'], n_knots=pl['n_knots'], n_samp=10,
                                     max_updates=12, p_t=0, p_state0=1, p_input0=3, p_poseT=5, sample_time=0.01, inv_T=pl['inv_T'], stop_tol=1e-3))

    def rollout(pl):
        return C.byref(be.CRolloutSpec(n_steps=1, tau=d, t_rel=d, crossed=d, coeff_off=pl['coeff_off'], n_spl=pl['n_spl'], degree=pl['degree'],
                                       n_knots=pl['n_knots'], n_out=1, knots=kn(pl), p_off=d, p_t=-1, inv_T=pl['inv_T'], dt=0.1))

    def flat(pl):
        return pl['coeff_off'], pl['n_spl'], pl['degree'], kn(pl), pl['n_knots']
    return {
        'omgx_batch_sample': ('sample', 0, True, False, False, lambda pl: lib.omgx_batch_sample(None, d, *flat(pl), 1, d, 0.01, 5, d, 0, 0)),
        'omgx_batch_store': ('store', 1, True, False, True, lambda pl: lib.omgx_batch_store(None, d, store(pl))),
        'omgx_batch_set_store': ('store', 1, True, False, True, lambda pl: lib.omgx_batch_set_store(None, store(pl))),
        'omgx_batch_set_signals': ('signals', 1, True, False, True, lambda pl: lib.omgx_batch_set_signals(None, signals(pl))),
        'omgx_batch_signals_append': ('signals', 1, True, False, True, lambda pl: lib.omgx_batch_signals_append(None, d, d, None, signals(pl))),
        'omgx_batch_signals_reduce': ('signals', 1, True, False, True, lambda pl: lib.omgx_batch_signals_reduce(None, signals(pl), d, d)),
        'omgx_batch_set_plant': ('plant', 1, True, True, True, lambda pl: lib.omgx_batch_set_plant(None, plant(pl), None)),
        'omgx_batch_plant_simulate': ('plant', 1, True, True, True, lambda pl: lib.omgx_batch_plant_simulate(None, d, d, plant(pl), None)),
        'omgx_batch_plant_predict': ('plant', 1, True, True, True, lambda pl: lib.omgx_batch_plant_predict(None, d, d, 0.1, 0.1, plant(pl))),
        'omgx_batch_predict': ('predict', 1, True, False, True,
                               lambda pl: lib.omgx_batch_predict(None, d, d, *flat(pl), 0.1, pl['inv_T'], 0, 2, -1, 0.0)),
        'omgx_batch_predict_ex': ('predict', 1, True, False, True,
                                  lambda pl: lib.omgx_batch_predict_ex(None, d, d, *flat(pl), 0.1, pl['inv_T'], 1, d, -1, 0.0, 0, None, 0, 0.0)),
        'omgx_batch_predict_quadrotor': ('predict_quadrotor', 3, False, False, True,
                                         lambda pl: lib.omgx_batch_predict_quadrotor(None, d, d, pl['coeff_off'], pl['degree'], kn(pl), pl['n_knots'], 0.1,
                                                                                     pl['inv_T'], 1, d, -1, 0.0, d, None, 1, 0.01, 9.81)),
        'omgx_batch_rollout': ('rollout', 1, True, True, True, lambda pl: lib.omgx_batch_rollout(None, rollout(pl), d, d, d, d, d, d, d, dev)),
    }, lib, (mem, knots)


def test_every_plan_taking_entry_holds_the_plan_to_the_one_rule():
    entries, lib, keep = _entries()
    assert len(entries) == 13
    for name, (who, min_degree, has_n_spl, owned_spl, has_inv_T, call) in entries.items():
        def refused(field, **change):
            rc = call(dict(PLAN, **change))
            msg = lib.omgx_last_error()
            assert rc == INVALID and msg.startswith(who.encode() + b':') and field in msg, (name, change, rc, msg)
        assert call(dict(PLAN)) == INVALID and b'null handle' in lib.omgx_last_error(), (name, lib.omgx_last_error())
        refused(b'n_knots', n_knots=41)
        refused(b'n_knots', n_knots=2 * PLAN['degree'] + 1)
        refused(b'degree', degree=6)
        refused(b'degree', degree=min_degree - 1)
        refused(b'coeff_off', coeff_off=-1)
        refused(b'knots', knots=False)
        if has_n_spl:
            refused(b'n_spl', n_spl=0)
        if has_inv_T:
            refused(b'inv_T', inv_T=0.0)
        if owned_spl:                                      # (a thread owns a spline: at most one wave of them)
            refused(b'n_spl', n_spl=65)
        elif has_n_spl:
            assert call(dict(PLAN, n_spl=65)) == INVALID and b'null handle' in lib.omgx_last_error(), name
        if min_degree == 0:                                # (omgx_batch_sample evaluates piecewise constants too)
            assert call(dict(PLAN, degree=0)) == INVALID and b'null handle' in lib.omgx_last_error(), name
        else:
            refused(b'degree', degree=0)
    del keep
