!  qn_shift_dev -- qn_shift_dev's loop (the reference's test/driver2.f90:66-195 on device buffers, the library's
!  built-in separable bounded quadratic, classic entry setulb_dev) to a NEW_X return, then the model on the free
!  variables: the rows that lbfgsb_kkt reports at a bound (codes 1, 2, 3) are pinned (d_i = +inf), the others get
!  d_i = 0 (lbfgsb_qn_shift_set with mu = 0).  Prints log det of B on the free rows (lbfgsb_qn_shift_logdet) and, for
!  v = 1 on every row, the residual |(B + D) x - v| over the free rows of x = lbfgsb_qn_shift_solve(v), with B x from
!  lbfgsb_qn_apply (x is +0 on the pinned rows, so rows F of B x are B_FF x_F).
!
!     qn_shift_dev [n [m [iterations]]]      defaults 100000, 5, 12
!
!  Output: one "Iterate" line per iterate, then
!     QNSHIFT col = <stored pairs> pinned = <pinned rows>
!     QNSHIFT logdet <log det of the shifted model on the free rows>
!     QNSHIFT residual <|(B + D) x - v| over the free rows> <|v| over the free rows> <largest |x| on a pinned row>
      program qn_shift_dev

      use lbfgsb_module, wp => lbfgsp_wp
      use iso_c_binding
      use iso_fortran_env, only: output_unit
      use, intrinsic :: ieee_arithmetic, only: ieee_value, ieee_positive_inf

      implicit none

      interface
         function hipMalloc(ptr, nbytes) bind(C, name='hipMalloc') result(rc)
            import :: c_ptr, c_size_t, c_int
            type(c_ptr) :: ptr
            integer(c_size_t), value :: nbytes
            integer(c_int) :: rc
         end function hipMalloc
         function hipFree(ptr) bind(C, name='hipFree') result(rc)
            import :: c_ptr, c_int
            type(c_ptr), value :: ptr
            integer(c_int) :: rc
         end function hipFree
         function hipMemcpy(dst, src, nbytes, kind) bind(C, name='hipMemcpy') result(rc)
            import :: c_ptr, c_size_t, c_int
            type(c_ptr), value :: dst, src
            integer(c_size_t), value :: nbytes
            integer(c_int), value :: kind
            integer(c_int) :: rc
         end function hipMemcpy
         function hipMemset(dst, val, nbytes) bind(C, name='hipMemset') result(rc)
            import :: c_ptr, c_size_t, c_int
            type(c_ptr), value :: dst
            integer(c_int), value :: val
            integer(c_size_t), value :: nbytes
            integer(c_int) :: rc
         end function hipMemset
      end interface
      integer(c_int), parameter :: H2D = 1, D2H = 2

      integer               :: n, m, maxit, rc, i
      real(wp), parameter   :: factr = 0.0_wp, pgtol = 0.0_wp
      character(len=60)     :: task, csave
      character(len=32)     :: arg
      logical               :: lsave(4)
      integer               :: isave(44)
      real(wp)              :: f, dsave(29)
      real(c_double)        :: logdet, res, vnorm, xpin, ri
      type(c_ptr)           :: ctx, dx, dg, dl, du, dnbd, du1, dhu, dd, dstatus
      real(wp), allocatable, target :: hu(:), hd(:)
      integer(c_int8_t), allocatable, target :: hstatus(:)
      integer(c_int64_t)    :: cnt(LBFGSB_KKT_NCNT), pinned
      real(c_double)        :: val(LBFGSB_KKT_NVAL)
      real(wp), allocatable, target :: hbuf(:)
      integer(c_int32_t), allocatable, target :: hnbd(:)
      integer(c_size_t)     :: vbytes

      n = 100000; m = 5; maxit = 12
      if (command_argument_count() >= 1) then
         call get_command_argument(1, arg); read (arg, *) n
      end if
      if (command_argument_count() >= 2) then
         call get_command_argument(2, arg); read (arg, *) m
      end if
      if (command_argument_count() >= 3) then
         call get_command_argument(3, arg); read (arg, *) maxit
      end if

      vbytes = int(n, c_size_t)*int(storage_size(1.0_wp)/8, c_size_t)
      call chk(hipMalloc(dx, vbytes), 'hipMalloc x')
      call chk(hipMalloc(dg, vbytes), 'hipMalloc g')
      call chk(hipMalloc(dl, vbytes), 'hipMalloc l')
      call chk(hipMalloc(du, vbytes), 'hipMalloc u')
      call chk(hipMalloc(du1, vbytes), 'hipMalloc u')
      call chk(hipMalloc(dhu, vbytes), 'hipMalloc H u')
      call chk(hipMalloc(dd, vbytes), 'hipMalloc d')
      call chk(hipMalloc(dstatus, int(n, c_size_t)), 'hipMalloc status')
      call chk(hipMalloc(dnbd, int(n, c_size_t)*4_c_size_t), 'hipMalloc nbd')
      call chk(hipMemset(dx, 0_c_int, vbytes), 'hipMemset x')             ! x0 = 0
      call chk(hipMemset(dg, 0_c_int, vbytes), 'hipMemset g')
      allocate (hbuf(n))
      hbuf = -1.0_wp                                                       ! l = -1
      call chk(hipMemcpy(dl, c_loc(hbuf), vbytes, H2D), 'hipMemcpy l')
      hbuf = 1.0_wp                                                        ! u = +1
      call chk(hipMemcpy(du, c_loc(hbuf), vbytes, H2D), 'hipMemcpy u')
      allocate (hnbd(n))
      do i = 1, n
         hnbd(i) = int(mod(i, 4), c_int32_t)                               ! all four bound types
      end do
      call chk(hipMemcpy(dnbd, c_loc(hnbd), int(n, c_size_t)*4_c_size_t, H2D), 'hipMemcpy nbd')
      deallocate (hnbd)

      call lbfgsb_create(ctx, n, m, 0, rc)
      if (rc /= 0) then
         write (output_unit, '(2a)') ' lbfgsb_create failed: ', lbfgsb_error_message()
         error stop 1
      end if

      task = 'START'
      f = 0.0_wp
      do while (task(1:2) == 'FG' .or. task == 'NEW_X' .or. task == 'START')
         call setulb_dev(ctx, dx, dl, du, dnbd, f, dg, factr, pgtol, task, -1, csave, lsave, isave, dsave, rc)
         if (rc /= 0) then
            write (output_unit, '(2a)') ' setulb_dev failed: ', lbfgsb_error_message()
            error stop 1
         end if
         if (task(1:2) == 'FG') then
            call lbfgsb_objective(ctx, 0, dx, dg, rc, f)
            if (rc /= 0) error stop 2
         else if (task(1:5) == 'NEW_X') then
            write (output_unit, '(2(a,i5,4x),a,1p,d12.5,4x,a,1p,d12.5)') 'Iterate', isave(30), 'nfg =', isave(34), &
               'f =', f, '|proj g| =', dsave(13)
            if (isave(30) >= maxit) exit                                   ! the model of this NEW_X return
         end if
      end do

      ! the rows at a bound at this iterate (codes 1, 2, 3 of lbfgsb_kkt's status) are pinned, the others not shifted
      call lbfgsb_kkt(ctx, dx, dl, du, dnbd, dg, 0.0_c_double, c_null_ptr, c_null_ptr, dstatus, cnt, val, rc)
      if (rc /= 0) then
         write (output_unit, '(2a)') ' lbfgsb_kkt failed: ', lbfgsb_error_message()
         error stop 1
      end if
      allocate (hstatus(n), hd(n), hu(n))
      call chk(hipMemcpy(c_loc(hstatus), dstatus, int(n, c_size_t), D2H), 'hipMemcpy status')
      do i = 1, n
         if (hstatus(i) >= 1_c_int8_t) then
            hd(i) = ieee_value(1.0_wp, ieee_positive_inf)
         else
            hd(i) = 0.0_wp
         end if
      end do
      call chk(hipMemcpy(dd, c_loc(hd), vbytes, H2D), 'hipMemcpy d')
      call lbfgsb_qn_shift_set(ctx, dd, 0.0_c_double, pinned, rc)
      if (rc == 0) call lbfgsb_qn_shift_logdet(ctx, logdet, rc)
      if (rc /= 0) then
         write (output_unit, '(2a)') ' lbfgsb_qn_shift_set / _logdet failed: ', lbfgsb_error_message()
         error stop 1
      end if
      write (output_unit, '(a,i4,a,i0)') 'QNSHIFT col =', isave(28), ' pinned = ', pinned
      write (output_unit, '(a,es25.16e3)') 'QNSHIFT logdet', logdet
      ! x = (B + D)^-1 v on the free rows for v = 1, then B x by the model itself
      hbuf = 1.0_wp
      call chk(hipMemcpy(du, c_loc(hbuf), vbytes, H2D), 'hipMemcpy v')
      call lbfgsb_qn_shift_solve(ctx, 1, du, n, du1, n, rc)
      if (rc == 0) call lbfgsb_qn_apply(ctx, LBFGSB_QN_B, 1, du1, n, dhu, n, rc)
      if (rc /= 0) then
         write (output_unit, '(2a)') ' lbfgsb_qn_shift_solve / lbfgsb_qn_apply failed: ', lbfgsb_error_message()
         error stop 1
      end if
      call chk(hipMemcpy(c_loc(hu), du1, vbytes, D2H), 'hipMemcpy x')
      call chk(hipMemcpy(c_loc(hbuf), dhu, vbytes, D2H), 'hipMemcpy B x')
      res = 0.0_c_double; vnorm = 0.0_c_double; xpin = 0.0_c_double
      do i = 1, n
         if (hstatus(i) >= 1_c_int8_t) then
            xpin = max(xpin, abs(real(hu(i), c_double)))
         else
            ri = real(hbuf(i), c_double) + real(hd(i), c_double)*real(hu(i), c_double) - 1.0_c_double
            res = res + ri**2
            vnorm = vnorm + 1.0_c_double
         end if
      end do
      write (output_unit, '(a,3es25.16e3)') 'QNSHIFT residual', sqrt(res), sqrt(vnorm), xpin
      deallocate (hstatus, hd, hu)

      task = 'STOP: QN_SHIFT_DEV'
      call lbfgsb_destroy(ctx)
      rc = hipFree(dx); rc = hipFree(dg); rc = hipFree(dl); rc = hipFree(du)
      rc = hipFree(du1); rc = hipFree(dnbd); rc = hipFree(dhu); rc = hipFree(dd); rc = hipFree(dstatus)

      contains

      subroutine chk(code, what)
      integer(c_int), intent(in) :: code
      character(len=*), intent(in) :: what
      if (code /= 0) then
         write (output_unit, '(3a,i0)') ' ', what, ' failed, hipError ', code
         error stop 3
      end if
      end subroutine chk

      end program qn_shift_dev
