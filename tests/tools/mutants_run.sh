python "$(dirname "$0")/mutants.py" run kernels "$@"
