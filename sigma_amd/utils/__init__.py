"""Stand-ins for pieces of the reference's ``utils/`` that do not run as they are on the torch this project uses:
``loss_opr.ProbOhemCrossEntropy2d``; and for one that the kernels take over: ``loss_opr.FocalLoss2d``."""
