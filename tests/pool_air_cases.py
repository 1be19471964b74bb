"""What tests/test_pool_air_cpu.py and tests/test_gpu_pool_air.py share: the statements of bfhip_pool_submit_air's tests without their device
columns (host only), built from the programs of tests/test_gpu_air_prove.py."""
from test_gpu_air_prove import _lookup_programs, _lookup_rules, _lookup_statement, _shift_program      # noqa: F401  (re-exported)


def shapes_statement(pkg, L):
    """The four-component statement of test_gpu_air_prove._shapes, the statement alone: tree 0 as coefficients (IsFirst(L), IsFirst(L + 1),
    a column nobody binds), tree 1 behind two mixed words (lookup A and the seven columns of the shift AIR), tree 2 behind one (lookup B at
    L + 1, lookup C at L); the shift AIR at log_expand 2 between components with fractions; two relations."""
    S = pkg.AirStatement
    program, fractions = _lookup_programs(pkg)
    st = S(n_relations=2)
    t0 = st.tree([L, L + 1, L], form=1)
    t1 = st.tree([L] * 10, mix_u64=[7, (1 << 40) + 3])
    t2 = st.tree([L + 1] * 3 + [L] * 3, mix_u64=[11])
    inter = [(S.INTERACTION, j) for j in range(8)]
    st.component(program, L, 1, [(t1, 0), (t1, 1), (t1, 2), (t0, 0)] + inter, _lookup_rules(pkg, 0), fractions=fractions, fraction_columns=[(t1, 0), (t1, 1), (t1, 2)])
    st.component(_shift_program(pkg), L, 2, [(t1, 3 + c) for c in range(7)], [])
    st.component(program, L + 1, 1, [(t2, 0), (t2, 1), (t2, 2), (t0, 1)] + inter, _lookup_rules(pkg, 1), fractions=fractions, fraction_columns=[(t2, 0), (t2, 1), (t2, 2)])
    st.component(program, L, 1, [(t2, 3), (t2, 4), (t2, 5), (t0, 0)] + inter, _lookup_rules(pkg, 0), fractions=fractions, fraction_columns=[(t2, 3), (t2, 4), (t2, 5)])
    return st
