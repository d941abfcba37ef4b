"""python -m cytospace_amd -sp ... -ctp ... -stp ... -cp ... (-ctfep ... | -stctp ...): the CytoSPACE command line."""
from .cytospace import run_cytospace

if __name__ == "__main__":
    run_cytospace()
