# timing knock-outs of an attention tile loop (results are garbage): which part of the loop the time follows.  One library per mask.
#   bash tools/ab_attn_knockouts.sh x2f  > profiles/<name>.txt     the f16x2 forward        (-DLA_X2F_KO=<mask>,  kbench attn_fwd)
#   bash tools/ab_attn_knockouts.sh attn > profiles/<name>.txt     the 16-bit kernel        (-DLA_ATTN_KO=<mask>, kbench attn_ko)
#   build (no GPU needed):  for k in 1 6 8 16 17 32 30; do bash tools/build_variant.sh x2fko$k -DLA_X2F_KO=$k; done      (attnko$k -DLA_ATTN_KO=$k)
# masks: 1 exponentials, 2 V^T fragment reads, 4 K fragment reads, 8 staging, 16 MFMAs, 32 the tile barrier
case "$1" in
  x2f)  tag=x2fko;  run() { KB_BIG_ONLY=1 python tools/kbench.py attn_fwd --iters 20 2>&1 | grep "attn fwd"; } ;;
  attn) tag=attnko; run() { python tools/kbench.py attn_ko --iters 20 2>&1 | grep "attention"; } ;;
  *) echo "usage: $0 x2f|attn" >&2; exit 2 ;;
esac
echo "shipped"; run
for k in 1 6 8 16 17 32 30; do
  [ -f ab/$tag$k/liblyricalign_hip.so ] || continue
  echo "knock-out $k"; LA_LIB_PATH=ab/$tag$k/liblyricalign_hip.so run
done
