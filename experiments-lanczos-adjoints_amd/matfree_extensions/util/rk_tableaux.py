"""Butcher tableaux of the fixed-step explicit Runge-Kutta baselines of the PDE work-precision study (``pde_util.solver_rk``).

``get(name)`` -> ``Tableau(name, order, a, b)`` with ``a`` strictly lower triangular (row i holds the i coefficients a_i0 .. a_i,i-1)
and ``b`` the weights of the propagated solution.  ``get`` serves the fixed-step solves: no embedded error estimators, no dense output.
``get_pair(name)`` -> ``Pair(name, order, tab, e)`` serves ``pde_util.solver_rk_adaptive``: ``tab`` the propagated method, ``e = b - bhat``
the error weights (the local error estimate of a step is h sum_i e_i K_i) and ``order`` the controller's exponent (the order of the
error estimator + 1).  The pairs: dopri5 (e = scipy 1.15's ``RK45.E``), bosh3 (Bogacki & Shampine 1989; scipy's ``RK23`` A, B, E with the
fourth stage row equal to B, the stage scipy evaluates as f(y+)), heun (Heun's method with its embedded Euler step).  dopri8 is refused:
DOP853 estimates its error from two formulae, which is another controller.

  euler, heun (explicit trapezoid), midpoint, rk4   the textbook coefficients
  dopri5   Dormand & Prince (1980), "A family of embedded Runge-Kutta formulae", J. Comput. Appl. Math. 6: the 5th-order solution
           of the 5(4) pair (7 stages; the last one is the first of the next step and has weight 0)
  dopri8   the 12 stages of the 8th-order solution of DOP853 (Hairer, Norsett & Wanner, Solving ODEs I), the values of scipy 1.15's
           scipy.integrate._ivp.dop853_coefficients (A[:12, :12], B), copied here: nothing is imported at run time
  tsit5    NOT AVAILABLE: no dependency of this package carries Tsitouras' coefficients, and they are not retyped from
           memory; the name raises NotImplementedError
"""

from __future__ import annotations

import collections

from .. import _lib

Tableau = collections.namedtuple("Tableau", "name order a b")

_DOPRI5_A = (
    (),
    (1 / 5,),
    (3 / 40, 9 / 40),
    (44 / 45, -56 / 15, 32 / 9),
    (19372 / 6561, -25360 / 2187, 64448 / 6561, -212 / 729),
    (9017 / 3168, -355 / 33, 46732 / 5247, 49 / 176, -5103 / 18656),
    (35 / 384, 0.0, 500 / 1113, 125 / 192, -2187 / 6784, 11 / 84),
)
_DOPRI5_B = (35 / 384, 0.0, 500 / 1113, 125 / 192, -2187 / 6784, 11 / 84, 0.0)

_DOPRI8_A = (
    (),
    (0.05260015195876773,),
    (0.0197250569845379, 0.0591751709536137),
    (0.02958758547680685, 0.0, 0.08876275643042054),
    (0.2413651341592667, 0.0, -0.8845494793282861, 0.924834003261792),
    (0.037037037037037035, 0.0, 0.0, 0.17082860872947386, 0.12546768756682242),
    (0.037109375, 0.0, 0.0, 0.17025221101954405, 0.06021653898045596, -0.017578125),
    (0.03709200011850479, 0.0, 0.0, 0.17038392571223998, 0.10726203044637328, -0.015319437748624402, 0.008273789163814023),
    (0.6241109587160757, 0.0, 0.0, -3.3608926294469414, -0.868219346841726, 27.59209969944671, 20.154067550477894, -43.48988418106996),
    (0.47766253643826434, 0.0, 0.0, -2.4881146199716677, -0.590290826836843, 21.230051448181193, 15.279233632882423, -33.28821096898486, -0.020331201708508627),
    (-0.9371424300859873, 0.0, 0.0, 5.186372428844064, 1.0914373489967295, -8.149787010746927, -18.52006565999696, 22.739487099350505, 2.4936055526796523, -3.0467644718982196),
    (2.273310147516538, 0.0, 0.0, -10.53449546673725, -2.0008720582248625, -17.9589318631188, 27.94888452941996, -2.8589982771350235, -8.87285693353063, 12.360567175794303, 0.6433927460157636),
)
_DOPRI8_B = (0.054293734116568765, 0.0, 0.0, 0.0, 0.0, 4.450312892752409, 1.8915178993145003, -5.801203960010585, 0.3111643669578199, -0.1521609496625161, 0.20136540080403034, 0.04471061572777259)

_TABLEAUX = {
    "euler": Tableau("euler", 1, ((),), (1.0,)),
    "heun": Tableau("heun", 2, ((), (1.0,)), (0.5, 0.5)),
    "midpoint": Tableau("midpoint", 2, ((), (0.5,)), (0.0, 1.0)),
    "rk4": Tableau("rk4", 4, ((), (0.5,), (0.0, 0.5), (0.0, 0.0, 1.0)), (1 / 6, 1 / 3, 1 / 3, 1 / 6)),
    "dopri5": Tableau("dopri5", 5, _DOPRI5_A, _DOPRI5_B),
    "dopri8": Tableau("dopri8", 8, _DOPRI8_A, _DOPRI8_B),
}
NAMES = tuple(_TABLEAUX)

Pair = collections.namedtuple("Pair", "name order tab e")

_DOPRI5_E = (-0.0012326388888888888, 0.0, 0.0042527702905061394, -0.03697916666666667, 0.05086379716981132, -0.0419047619047619, 0.025)
_BOSH3_B = (0.2222222222222222, 0.3333333333333333, 0.4444444444444444)
_BOSH3_E = (0.06944444444444445, -0.08333333333333333, -0.1111111111111111, 0.125)

_PAIRS = {
    "dopri5": Pair("dopri5", 5, _TABLEAUX["dopri5"], _DOPRI5_E),
    "bosh3": Pair("bosh3", 3, Tableau("bosh3", 3, ((), (0.5,), (0.0, 0.75), _BOSH3_B), _BOSH3_B + (0.0,)), _BOSH3_E),
    "heun": Pair("heun", 2, _TABLEAUX["heun"], (-0.5, 0.5)),
}
PAIR_NAMES = tuple(_PAIRS)


def get(name):
    if name == "tsit5":
        raise NotImplementedError("tsit5: Tsitouras' 5(4) coefficients are not in any dependency of this package and are not "
                                  "retyped from memory; use dopri5 (the same order, one stage more)")
    if name not in _TABLEAUX:
        raise ValueError(f"unknown Runge-Kutta method {name!r}: one of {NAMES}")
    return _TABLEAUX[name]


def struct(tab):
    """``struct mfx_rk_tableau`` of a Tableau (zero-filled beyond its stages)"""
    out = _lib.RkTableau()
    out.stages = len(tab.b)
    for i, row in enumerate(tab.a):
        for j, v in enumerate(row):
            out.a[i][j] = float(v)
    for i, v in enumerate(tab.b):
        out.b[i] = float(v)
    return out


def get_pair(name):
    if name == "dopri8":
        raise NotImplementedError("dopri8 has no embedded pair here: DOP853 combines two error estimators, which is a different "
                                  f"controller; one of {PAIR_NAMES}")
    if name not in _PAIRS:
        raise ValueError(f"unknown embedded Runge-Kutta pair {name!r}: one of {PAIR_NAMES}")
    return _PAIRS[name]


def pair_struct(pair):
    """``struct mfx_rk_pair`` of a Pair"""
    out = _lib.RkPair()
    out.tab = struct(pair.tab)
    for i, v in enumerate(pair.e):
        out.e[i] = float(v)
    out.order = int(pair.order)
    return out
