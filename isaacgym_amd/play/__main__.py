"""python -m isaacgym_amd.play"""
from .cli import main

main()
