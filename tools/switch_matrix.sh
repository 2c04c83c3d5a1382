#!/bin/bash
# The -m gpu suite once per environment switch of the library (INTEGRATION.md "Environment switches"): every switch selects a form
# the tests must also pass on.  usage (through gpurun, at most four switches per call):  bash tools/switch_matrix.sh TAG VAR=VAL [VAR=VAL ...]
# Stops at the first run that timed out or crashed (exit 124, 134, 137, 139): nothing more is started on a card that may have faulted.
TAG=$1; shift
O=gpurun_out/switches_$TAG
mkdir -p $O
for sw in "$@"; do
  name=$(echo $sw | tr '=' '_')
  env $sw timeout -k 10 420 python -m pytest tests -q -m gpu -p no:cacheprovider > $O/$name.log 2>&1
  rc=$?
  echo "$sw: $(tail -1 $O/$name.log)" | tee -a $O/summary.txt
  case $rc in
    124|134|137|139)
      echo "$sw: stopped, the run exited with $rc (time limit or crash); the remaining switches were not run" | tee -a $O/summary.txt
      exit $rc ;;
  esac
done
