"""Replays tests/golden/option_grid.json (tests/golden/make_option_grid.py): every single generation option and every pair
of them, at every front door - the same refusal, word for word, or the same generator reached with the same options."""
import pytest

import make_option_grid as G

GRID = G.load()


@pytest.mark.parametrize('key', sorted(GRID))
def test_every_single_option_and_every_pair_does_what_was_recorded(key):
    kind, _, door = key.partition('/')
    make = G._kinds()[kind]
    assert set(GRID[key]) == {'+'.join(c) for c in G.CASES}
    wrong = []
    for case in G.CASES:
        want = dict(GRID[key]['+'.join(case)])
        either = want.pop('first_of', None)
        got = G.run_case(make, kind, case, door or 'generate')
        if either is not None:                                # two refusals apply: either may speak, the class is fixed
            ok = got.get('error') == want['error'] and got.get('message') in either
        else:
            ok = got == want
        if not ok:
            wrong.append((case, want, got))
    assert not wrong, '%d of %d cases differ, the first: %r' % (len(wrong), len(G.CASES), wrong[0])


def test_the_cases_that_accept_either_message_are_a_minority_of_the_refused_pairs():
    doors = ('transformer_glove', 'dynconv/lanes', 'lstm_decoder/lanes')
    pairs = [r for key in doors for case, r in GRID[key].items() if case.count('+') == 1 and 'error' in r]
    either = [r for key in GRID for r in GRID[key].values() if 'first_of' in r]
    assert all('first_of' not in r for key in GRID if key not in doors for r in GRID[key].values())
    assert 0 < len(either) < len(pairs) / 2, (len(either), len(pairs))
