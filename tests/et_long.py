"""A long synthetic ET-prelude sequence through the public shud_et_step inputs (shared by tests/test_et.py on the
CPU and tests/test_gpu_et.py on the device).  It reaches what the short sequences never do:

* the day-mean queues fill and pop: ft_surf_day = 2, ft_sub_day = 3 and seven day pushes, with step lengths that
  do not divide 1440 min, so the number of samples in a day mean changes from day to day and the ring
  (capacity days + 1) wraps;
* exact thresholds: the last station has NA elevation, so t_temp == its TMP exactly, and its TMP walks through
  Tsnow = -3, To = 0 and Train = 1 and the doubles next to them (FrozenFraction's T > high / T < low, melt's T > To);
  elements whose own z_surf is NA_VALUE take the other stations' TMP unchanged (ifequal(z, NA_VALUE));
* interception storage above its capacity (icStg > icMax), melt limited by snStg / DT;
* a CACHED terrain-radiation step before any RECOMPUTE, and an all-night RECOMPUTE (tsr_den == 0)."""
import numpy as np

from shud_rhs import abi, et

DTS = [420.0, 250.0, 610.0, 335.0, 180.0, 500.0]     # minutes; day pushes at steps 0, 4, 9, 14, 18, 22, 27
N_STEPS = 28                                            # ~7.9 days: seven day pushes
_W = [-3.0, 0.0, 1.0]
WALK = [v for c in _W for v in (c, np.nextafter(c, -np.inf), np.nextafter(c, np.inf))] + [0.5, -1.0, 12.0]
SIZES = [1, 63, 257]                                    # plus one mesh of a few thousand elements in each test
EXACT = ["t_prcp", "t_temp", "t_lai", "t_mf", "t_rn", "t_wind", "t_rh", "rn_factor", "yEleSnow", "fu_surf", "fu_sub"]


def et_model(n, seed=21):
    etm = et.synth_et(n, seed=seed, terrain=True, lake_frac=0.04)
    a = etm.arrays
    k = np.arange(n)
    a["iforc"] = np.where(k % 3 == 0, 3, a["iforc"]).astype(np.int64)       # a third of the mesh on the NA station
    a["z_surf"] = np.where(k % 7 == 1, -9999.0, a["z_surf"])                # the element's own elevation is NA
    a["fix_pressure"] = et.pressure_elevation(np.where(k % 7 == 1, 500.0, a["z_surf"]))
    etm.params.update(cryosphere=1, ft_surf_day=2, ft_sub_day=3, ft_surf_max=2.0, ft_surf_min=-4.0,
                      ft_sub_max=1.5, ft_sub_min=-2.5)
    rng = np.random.default_rng(seed + 1)
    y_is = rng.uniform(0, 2e-4, n)
    y_is[k % 5 == 2] = 5e-3                                                 # far above icMax = 2e-4 * LAI
    y_snow = np.where(rng.random(n) < 0.5, 0.0, rng.uniform(0, 0.05, n))
    y_snow[k % 4 == 3] = 1e-7                                               # melts away within a step: snStg / DT
    return etm, y_is, y_snow


def forcings(first_cached=True):
    """first_cached: step 0 is a CACHED terrain-radiation step before any RECOMPUTE (the CPU restatements take it
    as a factor of 0; the device handle refuses it, so the GPU test passes False: step 0 is then an all-night
    RECOMPUTE, which gives the same factor 0)"""
    out, t = [], 0.0
    for k in range(N_STEPS):
        dt = DTS[k % len(DTS)]
        mode = abi.SHUD_TSR_RECOMPUTE if k % 4 == 1 else abi.SHUD_TSR_CACHED      # k = 0: CACHED before any RECOMPUTE
        if k == 6:
            mode = abi.SHUD_TSR_NO_TIME
        if k == 0 and not first_cached:
            mode = abi.SHUD_TSR_RECOMPUTE
        f = et.synth_forcing(t, dt, seed=100 + k, tsr_mode=mode)
        st = f.station.copy()
        st[3, 1] = [12.0, 0.0, 40.0][k % 3]                                  # rain / snow on the walking station
        st[3, 2] = WALK[k % len(WALK)]
        st[2, 2] = 6.0 + (k % 5)                                             # a warm station: melt > snStg / DT
        f.station = st
        if k == 9 or (k == 0 and not first_cached):                          # all-night interval: no weight at all
            assert mode == abi.SHUD_TSR_RECOMPUTE
            f.tsr[2] = -np.abs(f.tsr[2]) - 0.01
            f.tsr[3] = 0.0
            f.tsr_den = 0.0
        out.append(f)
        t += dt
    return out
