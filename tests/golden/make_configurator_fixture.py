"""What the reference's own util/configurator.py makes of its unchanged NeuRec.properties and
conf/{MF,LightGCN,NGCF,MultiVAE}.properties (copied, settings only, to tests/golden/neurec_conf/), for
`main.py --recommender=<Model> --num_thread=4`: every key in order with its value's type and repr,
params_str() and str().  Written to tests/golden/configurator_reference.json.

    python tests/golden/make_configurator_fixture.py       # needs the reference tree (oracle/ref_models.REF)
"""
import importlib.util
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CONF_DIR = os.path.join(HERE, "neurec_conf")
MODELS = ("MF", "LightGCN", "NGCF", "MultiVAE")


def record(conf):
    keys = list(conf.lib_arg) + list(conf.alg_arg)
    return {"keys": keys, "values": {k: [type(conf[k]).__name__, repr(conf[k])] for k in keys},
            "params_str": conf.params_str(), "str": str(conf)}


def main():
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    from oracle.ref_models import REF
    spec = importlib.util.spec_from_file_location("ref_configurator", os.path.join(REF, "util", "configurator.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    cwd, argv = os.getcwd(), sys.argv
    out = {}
    os.chdir(CONF_DIR)
    try:
        for model in MODELS:
            sys.argv = ["main.py", "--recommender=%s" % model, "--num_thread=4"]
            out[model] = record(mod.Configurator("NeuRec.properties", default_section="hyperparameters"))
    finally:
        os.chdir(cwd)
        sys.argv = argv
    with open(os.path.join(HERE, "configurator_reference.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print({m: len(v["keys"]) for m, v in out.items()})


if __name__ == "__main__":
    main()
