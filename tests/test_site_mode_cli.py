"""--site_proba on `inference` and `eventalign_inference`: listed by --help, refused with status 2 for any other value, carried
to the ranks of --gpus N, and absent from the parsers the two commands share with each other.  No GPU."""
import pytest

from m6anet_amd import __main__ as cli
from m6anet_amd import multi_gpu
from m6anet_amd.scripts import eventalign_inference, inference

COMMANDS = {"inference": ["--input_dir", "d", "--out_dir", "o"], "eventalign_inference": ["--eventalign", "e.txt", "--out_dir", "o"]}


@pytest.mark.parametrize("command", sorted(COMMANDS))
def test_help_lists_site_proba(command, capsys):
    with pytest.raises(SystemExit) as e:
        cli.main([command, "--help"])
    assert e.value.code == 0
    text = " ".join(capsys.readouterr().out.split())
    assert "--site_proba {sampled,expected}" in text
    assert "--num_iterations and --seed have no effect" in text


@pytest.mark.parametrize("command", sorted(COMMANDS))
def test_any_other_value_is_an_argparse_error(command, capsys):
    with pytest.raises(SystemExit) as e:
        cli.main([command] + COMMANDS[command] + ["--site_proba", "nope"])
    assert e.value.code == 2
    assert "--site_proba" in capsys.readouterr().err


def test_default_is_sampled_and_the_shared_parsers_do_not_carry_the_flag():
    for mod, argv in ((inference, COMMANDS["inference"]), (eventalign_inference, COMMANDS["eventalign_inference"])):
        p = mod.command_parser()
        assert p.parse_args(argv).site_proba == "sampled"
        assert p.parse_args(argv + ["--site_proba", "expected"]).site_proba == "expected"
        flags = lambda q: {o for a in q._actions for o in a.option_strings}
        assert flags(p) - flags(mod.cli_parser()) == {"--site_proba"}
        assert "--site_proba" not in flags(mod.argparser())


def test_the_flag_reaches_every_rank():
    p = inference.command_parser()
    a = p.parse_args(COMMANDS["inference"] + ["--gpus", "2", "--site_proba", "expected"])
    assert vars(p.parse_args(multi_gpu.rank_argv(a))) == vars(a)
    b = p.parse_args(COMMANDS["inference"] + ["--gpus", "2"])
    assert "--site_proba" not in multi_gpu.rank_argv(b) and vars(p.parse_args(multi_gpu.rank_argv(b))) == vars(b)
