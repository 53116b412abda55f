"""loader.open_output: the text output of the command lines, a file or the standard output.  No GPU."""
import sys

import pytest

from explainn_amd.loader import open_output


@pytest.mark.parametrize("path", [None, ""])
def test_open_output_stdout(path, capsys):
    """Without a path: sys.stdout as it is when the block is entered (capsys has replaced it), left open."""
    with open_output(path) as fh:
        assert fh is sys.stdout
        fh.write("a row\n")
    assert not fh.closed
    fh.write("another\n")
    assert capsys.readouterr().out == "a row\nanother\n"


def test_open_output_file(tmp_path):
    path = tmp_path / "out.tsv"
    path.write_text("what an earlier run left, longer than the new text\n")
    with open_output(str(path)) as fh:
        assert fh is not sys.stdout
        fh.write("a row\n")
    assert fh.closed
    assert path.read_text() == "a row\n"


def test_open_output_file_closed_on_raise(tmp_path):
    path = tmp_path / "out.tsv"
    with pytest.raises(KeyError):
        with open_output(str(path)) as fh:
            fh.write("a row\n")
            raise KeyError("the body fails")
    assert fh.closed
    assert path.read_text() == "a row\n"


def test_open_output_stdout_open_on_raise(capsys):
    with pytest.raises(KeyError):
        with open_output(None) as fh:
            raise KeyError("the body fails")
    assert fh is sys.stdout and not fh.closed
