"""Dump the Python surface of the built extension: the pybind11 docstring (argument names, types, defaults) of every
public callable of deeplearning_mpi_amd._C and the value of every other public attribute.  Run in each tree after
`python -m deeplearning_mpi_amd.build --force`:  PYTHONPATH=. python profiles/binding_split/dump_surface.py > surface.json"""
import json
import sys

from deeplearning_mpi_amd._ext import native

C = native()
out = {}
for name in sorted(n for n in dir(C) if not n.startswith("_")):
    v = getattr(C, name)
    out[name] = v.__doc__ if callable(v) else repr(v)
json.dump(out, sys.stdout, indent=1, sort_keys=True)
print()
